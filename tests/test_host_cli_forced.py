"""The C++ host's and learn.py's --forced-k / --prune-target: forced playouts and policy target pruning in the self-play generation of
`-m learn`.  CPU part: the flags are listed, written to log/settings.txt, off by default, and a factor outside [0, 8], a switch that
is neither 0 nor 1, or pruning without forcing is rejected.  GPU part: a learn iteration with both runs to its end; pruning changes the
policies of the samples and nothing else."""
import pytest

import host_cli as H
from host_cli import exe  # noqa: F401  (a fixture)

FLAGS = ("--forced-k", "--prune-target")


def test_help_and_settings_file_carry_the_flags(exe, tmp_path):
    H.check_flags_carried(exe, tmp_path, FLAGS, ("2", "1"))


def test_the_defaults_are_off(exe, tmp_path):
    H.check_defaults(exe, tmp_path, FLAGS, ("0", "0"))


@pytest.mark.parametrize("bad", ["-0.5", "8.5", "nan", "x", ""])
def test_a_value_that_is_no_factor_is_rejected(exe, tmp_path, bad):
    H.check_host_rejects(exe, tmp_path, ["--forced-k=" + bad], "--forced-k")


@pytest.mark.parametrize("args", [["--forced-k=2", "--prune-target=2"], ["--forced-k=2", "--prune-target=x"], ["--prune-target=1"],
                                  ["--forced-k=0", "--prune-target=1"]])
def test_a_bad_switch_or_pruning_without_forcing_is_rejected(exe, tmp_path, args):
    H.check_host_rejects(exe, tmp_path, args, "--prune-target")


@pytest.mark.parametrize("args,flag", [(["--forced-k", "8.5"], "--forced-k"), (["--forced-k", "nan"], "--forced-k"),
                                       (["--forced-k", "-1"], "--forced-k"), (["--prune-target", "1"], "--prune-target"),
                                       (["--forced-k", "2", "--prune-target", "2"], "--prune-target")])
def test_learn_py_rejects_the_same_values(tmp_path, args, flag):
    H.check_learn_py_rejects(tmp_path, args, flag)


def test_learn_py_lists_the_flags():
    H.check_learn_py_lists(FLAGS, "[this build] self-play forced playouts", "[this build] self-play policy target pruning")


@pytest.mark.gpu
def test_learn_with_forcing_and_pruning(exe, tmp_path):
    plain = H.learn_records(exe, tmp_path / "plain").records
    forced = H.learn_records(exe, tmp_path / "forced", "--forced-k", "2").records
    pruned = H.learn_records(exe, tmp_path / "pruned", "--forced-k", "2", "--prune-target", "1").records
    assert forced.shape != plain.shape or (forced != plain).any()      # forcing changes the search, so the games
    # pruning keeps the games: the same self-play records outside pi (bytes 93..264)
    assert pruned.shape == forced.shape
    assert (forced[:, :93] == pruned[:, :93]).all() and (forced[:, 93:] != pruned[:, 93:]).any()
