"""The C++ host's and learn.py's --gumbel-m / --gumbel-cvisit / --gumbel-cscale / --gumbel-seed: the Gumbel root search in the
self-play generation of `-m learn`.  CPU part: the flags are listed, written to log/settings.txt, off by default, and a bad value is
rejected with the option's name.  GPU part: a learn iteration with the four flags runs to its end, says so in its log line, and writes
records whose pi is a softmax over the legal moves (no multiples of 1 / 16) — the flags reached the engine."""
import numpy as np
import pytest

import host_cli as H
from host_cli import exe  # noqa: F401  (a fixture)

FLAGS = ("--gumbel-m", "--gumbel-cvisit", "--gumbel-cscale", "--gumbel-seed")


def test_help_and_settings_file_carry_the_flags(exe, tmp_path):
    H.check_flags_carried(exe, tmp_path, FLAGS, ("8", "40", "0.25", "9"))


def test_the_default_is_off(exe, tmp_path):
    H.check_defaults(exe, tmp_path, FLAGS, ("0", "50", "0.5", "0"))


@pytest.mark.parametrize("arg", ["--gumbel-m=44", "--gumbel-m=-1", "--gumbel-m=x", "--gumbel-m=", "--gumbel-cvisit=-1", "--gumbel-cvisit=nan",
                                 "--gumbel-cscale=0", "--gumbel-cscale=inf", "--gumbel-cscale=x", "--gumbel-seed=-1", "--gumbel-seed=4294967296"])
def test_the_cli_rejects_a_bad_value(exe, tmp_path, arg):
    H.check_host_rejects(exe, tmp_path, [arg], arg.split("=")[0])


@pytest.mark.parametrize("args,why", [(("--gumbel-m", "44"), "is not a number of root moves"), (("--gumbel-cvisit", "-1"), "is not a c_visit"),
                                      (("--gumbel-cscale", "0"), "is not a c_scale"), (("--gumbel-cscale", "nan"), "is not a c_scale"),
                                      (("--gumbel-seed", "-1"), "is not a 32-bit seed"),
                                      (("--gumbel-m", "4", "--dir-alpha", "0.3"), "does not go with --dir-alpha")])
def test_learn_py_rejects_the_same_values(tmp_path, args, why):
    H.check_learn_py_rejects(tmp_path, args, args[0], why)


def test_learn_py_lists_the_flags():
    H.check_learn_py_lists(FLAGS, "[this build] self-play Gumbel root search")


@pytest.mark.gpu
def test_learn_with_the_gumbel_search(exe, tmp_path):
    run = H.learn_records(exe, tmp_path, "--gumbel-m", "4", "--gumbel-cvisit", "50", "--gumbel-cscale", "0.5", "--gumbel-seed", "9", mcts=16)
    assert "Gumbel root search: m 4, c_visit 50, c_scale 0.5, seed 9" in run.stdout
    pi = np.frombuffer(run.raw[8:], np.uint8).reshape(-1, 265)[:, 93:265].copy().view(np.float32)
    assert np.abs(pi.astype(np.float64).sum(1) - 1).max() <= 43 * 2.0 ** -24
    # the entries of a visit distribution over 16 simulations are multiples of 1/16; a softmax's are not
    assert (np.abs(pi * 16 - np.rint(pi * 16)) > 1e-3).any()
