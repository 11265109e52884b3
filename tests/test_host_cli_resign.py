"""The C++ host's and learn.py's --resign-q, --resign-streak, --resign-holdout and --resign-seed: resignation with a no-resign holdout
in the self-play generation of `-m learn`.  CPU part: the flags are listed, written to log/settings.txt, off by default, and a value
outside its range is rejected with the option's name.  GPU part: a learn iteration with resignation on runs to its end, prints the
statistics line and writes a well-formed data file."""
import re

import numpy as np
import pytest

import host_cli as H
from host_cli import exe  # noqa: F401  (a fixture)

FLAGS = ("--resign-q", "--resign-streak", "--resign-holdout", "--resign-seed")
STATS = r"Resignation: (\d+) resigned, (\d+) held out, (\d+) of them would have resigned, (\d+) of those did not lose  =>  false-positive share (\S+)"


def test_help_and_settings_file_carry_the_flags(exe, tmp_path):
    H.check_flags_carried(exe, tmp_path, FLAGS, ("-0.75", "3", "0.25", "11"))


def test_the_default_is_off(exe, tmp_path):
    H.check_defaults(exe, tmp_path, FLAGS, ("-0.9", "0", "0.1", "0"))


BAD = ["--resign-q=-1.5", "--resign-q=1.5", "--resign-q=nan", "--resign-q=x", "--resign-q=", "--resign-streak=-1", "--resign-streak=256",
       "--resign-streak=1.5", "--resign-streak=", "--resign-holdout=-0.1", "--resign-holdout=1.5", "--resign-holdout=nan",
       "--resign-seed=-1", "--resign-seed=4294967296", "--resign-seed=x"]


@pytest.mark.parametrize("arg", BAD)
def test_the_cli_rejects_a_bad_value(exe, tmp_path, arg):
    H.check_host_rejects(exe, tmp_path, [arg], arg.split("=")[0])


@pytest.mark.parametrize("flag,value", [("--resign-q", "-1.5"), ("--resign-q", "1.5"), ("--resign-q", "nan"), ("--resign-streak", "-1"),
                                        ("--resign-streak", "256"), ("--resign-holdout", "-0.1"), ("--resign-holdout", "1.5"),
                                        ("--resign-holdout", "nan"), ("--resign-seed", "-1"), ("--resign-seed", "4294967296")])
def test_learn_py_rejects_the_same_values(tmp_path, flag, value):
    H.check_learn_py_rejects(tmp_path, [flag + "=" + value], flag)


def test_learn_py_lists_the_flags():
    H.check_learn_py_lists(FLAGS, "[this build] self-play resignation")


@pytest.mark.gpu
def test_learn_with_resignation(exe, tmp_path):
    """every game held out, under the bound 1 that a root value of a running game lies below: all of them count, every one would have
    resigned at its first decision, and the false-positive share is that of the games the first mover did not lose"""
    run = H.learn_records(exe, tmp_path, "--resign-q", "1", "--resign-streak", "1", "--resign-holdout", "1", tg=4)
    m = re.search(STATS, run.stdout)
    assert m, run.stdout[-2000:]
    resigned, held, would, not_lost = (int(x) for x in m.groups()[:4])
    assert (resigned, held, would) == (0, 4, 4) and 0 <= not_lost <= 4 and float(m.group(5)) == not_lost / 4
    z = np.frombuffer(run.raw[8:], np.uint8).reshape(-1, 265)[:, 89:93].copy().view(np.float32)[:, 0]
    assert set(z.tolist()) <= {-1.0, 0.0, 1.0}
