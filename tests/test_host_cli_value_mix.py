"""The C++ host's and learn.py's --q-share: the value mix of the records in the self-play generation of `-m learn`.  CPU part: the flag
is listed, written to log/settings.txt, off by default, and a share outside [0, 1] is rejected with the option's name.  GPU part: a
learn iteration with the mix on runs to its end and writes a data file whose value targets are no longer all in {-1, 0, 1}."""
import numpy as np
import pytest

import host_cli as H
from host_cli import exe  # noqa: F401  (a fixture)

FLAG = "--q-share"


def test_help_and_settings_file_carry_the_flag(exe, tmp_path):
    H.check_flags_carried(exe, tmp_path, (FLAG,), ("0.25",))


def test_the_default_is_off(exe, tmp_path):
    H.check_defaults(exe, tmp_path, (FLAG,), ("0",))


@pytest.mark.parametrize("arg", ["--q-share=-0.5", "--q-share=1.5", "--q-share=nan", "--q-share=x", "--q-share="])
def test_the_cli_rejects_a_bad_value(exe, tmp_path, arg):
    H.check_host_rejects(exe, tmp_path, [arg], FLAG)


@pytest.mark.parametrize("value", ["-0.5", "1.5", "nan"])
def test_learn_py_rejects_the_same_values(tmp_path, value):
    H.check_learn_py_rejects(tmp_path, [FLAG, value], FLAG)


def test_learn_py_lists_the_flag():
    H.check_learn_py_lists((FLAG,), "[this build] self-play value mix")


@pytest.mark.gpu
def test_learn_with_the_value_mix(exe, tmp_path):
    raw = H.learn_records(exe, tmp_path, FLAG, "0.5").raw
    z = np.frombuffer(raw[8:], np.uint8).reshape(-1, 265)[:, 89:93].copy().view(np.float32)[:, 0]
    assert (np.abs(z) <= 1).all() and (~np.isin(z, [-1.0, 0.0, 1.0])).any()
