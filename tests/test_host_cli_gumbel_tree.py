"""The C++ host's and learn.py's --gumbel-tree: the Gumbel search's selection below the root in the self-play generation of `-m learn`.
CPU part: the flag is listed, written to log/settings.txt, off by default, a bad value is rejected with the option's name, and so is
the flag without --gumbel-m.  GPU part: a learn iteration with --gumbel-m 4 --gumbel-tree 1 runs to its end, says so behind the seed of
its log line, writes records whose pi sums to 1, and those records are not the ones of the same iteration without the flag — the
flag reached the engine."""
import numpy as np
import pytest

import host_cli as H
from host_cli import exe  # noqa: F401  (a fixture)

FLAGS = ("--gumbel-tree",)
LINE = "Gumbel root search: m 4, c_visit 50, c_scale 0.5, seed 9"
TAIL = ", improved-policy selection below the root"


def test_help_and_settings_file_carry_the_flag(exe, tmp_path):
    H.check_flags_carried(exe, tmp_path, FLAGS + ("--gumbel-m",), ("1", "4"))


def test_the_default_is_off(exe, tmp_path):
    H.check_defaults(exe, tmp_path, FLAGS, ("0",))


@pytest.mark.parametrize("arg", ["--gumbel-tree=2", "--gumbel-tree=-1", "--gumbel-tree=x", "--gumbel-tree="])
def test_the_cli_rejects_a_bad_value(exe, tmp_path, arg):
    H.check_host_rejects(exe, tmp_path, ["--gumbel-m=4", arg], "--gumbel-tree")


def test_the_cli_rejects_the_flag_without_the_root_search(exe, tmp_path):
    H.check_host_rejects(exe, tmp_path, ["--gumbel-tree=1"], "--gumbel-tree")
    H.check_host_rejects(exe, tmp_path, ["--gumbel-tree=1", "--gumbel-m=0"], "--gumbel-tree")


@pytest.mark.parametrize("args,why", [(("--gumbel-tree", "2", "--gumbel-m", "4"), "is not 0 or 1"), (("--gumbel-tree", "-1", "--gumbel-m", "4"), "is not 0 or 1"),
                                      (("--gumbel-tree", "1"), "needs the Gumbel root search"),
                                      (("--gumbel-tree", "1", "--gumbel-m", "0"), "needs the Gumbel root search")])
def test_learn_py_rejects_the_same(tmp_path, args, why):
    H.check_learn_py_rejects(tmp_path, args, "--gumbel-tree", why)


def test_learn_py_lists_the_flag():
    H.check_learn_py_lists(FLAGS, "[this build] under --gumbel-m,")


@pytest.mark.gpu
def test_learn_with_the_selection_below_the_root(exe, tmp_path):
    flags = ("--gumbel-m", "4", "--gumbel-cvisit", "50", "--gumbel-cscale", "0.5", "--gumbel-seed", "9")
    run = H.learn_records(exe, tmp_path / "tree", *flags, "--gumbel-tree", "1", mcts=16)
    assert LINE + TAIL in run.stdout
    pi = run.records[:, 93:265].copy().view(np.float32)
    assert np.abs(pi.astype(np.float64).sum(1) - 1).max() <= 43 * 2.0 ** -24
    plain = H.learn_records(exe, tmp_path / "plain", *flags, mcts=16)
    assert LINE in plain.stdout and TAIL not in plain.stdout
    assert plain.records.tobytes() != run.records.tobytes()
