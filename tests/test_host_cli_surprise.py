"""The C++ host's and learn.py's --psw-share / --psw-max / --psw-seed: policy surprise weighting of the records in the self-play
generation of `-m learn`.  CPU part: the flags are listed, written to log/settings.txt, off by default, and a share outside [0, 1], a
cap outside [1, 64] or a seed that is no 32-bit number is rejected.  GPU part: a learn iteration with weighting on runs to its end and
writes a data file."""
import pytest

import host_cli as H
from host_cli import exe  # noqa: F401  (a fixture)

FLAGS = ("--psw-share", "--psw-max", "--psw-seed")


def test_help_and_settings_file_carry_the_flags(exe, tmp_path):
    H.check_flags_carried(exe, tmp_path, FLAGS, ("0.5", "8", "77"))


def test_the_defaults_are_off(exe, tmp_path):
    H.check_defaults(exe, tmp_path, FLAGS, ("0", "4", "0"))


@pytest.mark.parametrize("arg", ["--psw-share=-0.5", "--psw-share=1.5", "--psw-share=nan", "--psw-share=x", "--psw-share=",
                                 "--psw-max=0.5", "--psw-max=65", "--psw-max=nan", "--psw-max=x", "--psw-max=",
                                 "--psw-seed=-1", "--psw-seed=4294967296", "--psw-seed=x", "--psw-seed="])
def test_the_cli_rejects_a_bad_value(exe, tmp_path, arg):
    H.check_host_rejects(exe, tmp_path, [arg], arg.split("=")[0])


@pytest.mark.parametrize("args", [["--psw-share", "-0.5"], ["--psw-share", "1.5"], ["--psw-share", "nan"], ["--psw-max", "0.5"],
                                  ["--psw-max", "65"], ["--psw-max", "nan"], ["--psw-seed", "-1"], ["--psw-seed", "4294967296"]])
def test_learn_py_rejects_the_same_values(tmp_path, args):
    H.check_learn_py_rejects(tmp_path, args, args[0])


def test_learn_py_lists_the_flags():
    H.check_learn_py_lists(FLAGS, "[this build] self-play policy surprise weighting")


@pytest.mark.gpu
def test_learn_with_surprise_weighting(exe, tmp_path):
    H.learn_records(exe, tmp_path, "--psw-share", "0.5")   # (asserts the run's end and the file's shape)
