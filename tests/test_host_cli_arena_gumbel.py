"""The C++ host's and learn.py's --arena-gumbel-m / -m2 / -tree / -tree2: the Gumbel search per side of the arena games (the compare and
benchmark games of `-m learn`, `-m play`).  CPU part: the flags are listed, written to log/settings.txt with the value in force —
player 2's is player 1's unless given —, off by default, a bad value is rejected with the option's name on both front ends, and so is a
tree flag without its m.  GPU part: `-m play --p1 az --p2 az --arena-gumbel-m 4` runs to its end and prints the log line."""
import subprocess

import pytest

import host_cli as H
from host_cli import exe  # noqa: F401  (a fixture)

FLAGS = ("--arena-gumbel-m", "--arena-gumbel-m2", "--arena-gumbel-tree", "--arena-gumbel-tree2")
NOT_M = "is not a number of root moves"


def test_help_and_settings_file_carry_the_flags(exe, tmp_path):
    H.check_flags_carried(exe, tmp_path, FLAGS, ("16", "3", "1", "0"))


def test_the_defaults_are_off(exe, tmp_path):
    H.check_defaults(exe, tmp_path, FLAGS, ("0", "0", "0", "0"))


def test_player_2_takes_player_1s_values_unless_given(exe, tmp_path):
    lines = H._settings(exe, tmp_path, "--arena-gumbel-m", "8", "--arena-gumbel-tree", "1")
    assert H.setting_values(lines, FLAGS) == [["8"], ["8"], ["1"], ["1"]]
    lines = H._settings(exe, tmp_path, "--arena-gumbel-m", "8", "--arena-gumbel-m2", "0", "--arena-gumbel-tree2", "0")
    assert H.setting_values(lines, FLAGS) == [["8"], ["0"], ["0"], ["0"]]


@pytest.mark.parametrize("flag", ["--arena-gumbel-m", "--arena-gumbel-m2"])
@pytest.mark.parametrize("value", ["44", "-1", "x", "", "2.5"])
def test_the_cli_rejects_a_bad_m(exe, tmp_path, flag, value):
    H.check_host_rejects(exe, tmp_path, [flag + "=" + value], flag)


@pytest.mark.parametrize("flag", ["--arena-gumbel-tree", "--arena-gumbel-tree2"])
@pytest.mark.parametrize("value", ["2", "-1", "x", ""])
def test_the_cli_rejects_a_bad_tree(exe, tmp_path, flag, value):
    H.check_host_rejects(exe, tmp_path, ["--arena-gumbel-m=4", flag + "=" + value], flag)


def test_the_cli_rejects_a_tree_without_its_m(exe, tmp_path):
    H.check_host_rejects(exe, tmp_path, ["--arena-gumbel-tree=1"], "--arena-gumbel-tree")
    H.check_host_rejects(exe, tmp_path, ["--arena-gumbel-tree=1", "--arena-gumbel-m=0", "--arena-gumbel-m2=4"], "--arena-gumbel-tree")
    H.check_host_rejects(exe, tmp_path, ["--arena-gumbel-m=4", "--arena-gumbel-m2=0", "--arena-gumbel-tree2=1"], "--arena-gumbel-tree2")


@pytest.mark.parametrize("args,flag,why", [
    (("--arena-gumbel-m", "44"), "--arena-gumbel-m", NOT_M), (("--arena-gumbel-m", "-1"), "--arena-gumbel-m", NOT_M),
    (("--arena-gumbel-m2", "44"), "--arena-gumbel-m2", NOT_M),
    (("--arena-gumbel-m", "4", "--arena-gumbel-tree", "2"), "--arena-gumbel-tree", "is not 0 or 1"),
    (("--arena-gumbel-m", "4", "--arena-gumbel-tree2", "-1"), "--arena-gumbel-tree2", "is not 0 or 1"),
    (("--arena-gumbel-tree", "1"), "--arena-gumbel-tree", "needs the Gumbel root search"),
    (("--arena-gumbel-m", "4", "--arena-gumbel-m2", "0", "--arena-gumbel-tree2", "1"), "--arena-gumbel-tree2", "needs the Gumbel root search")])
def test_learn_py_rejects_the_same(tmp_path, args, flag, why):
    H.check_learn_py_rejects(tmp_path, args, flag, why)


def test_learn_py_lists_the_flags():
    H.check_learn_py_lists(FLAGS, "[this build] compare and benchmark games:", "[this build] the same for player 2, the old net",
                           "[this build] under --arena-gumbel-m, player 1's", "[this build] the same for player 2 (default:")


@pytest.mark.gpu
def test_play_mode_with_a_gumbel_side(exe, tmp_path):
    r = subprocess.run([exe, "-m", "play", "--p1", "az", "--p2", "az", "--arena-gumbel-m", "4", "--mcts", "8", "--cg", "4", "--blocks", "1",
                        "--blocks2", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout[-2000:]
    assert r.stdout.count("Arena search: player 1 Gumbel m 4, player 2 Gumbel m 4\n") == 1
    tail = r.stdout.strip().split("\n")[-4:]
    assert tail[0] == "Games: 4"
    d, p1, p2 = (int(t.split(":")[1]) for t in tail[1:])
    assert d + p1 + p2 == 4
