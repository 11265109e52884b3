"""The C++ host's --cap-prob / --cap-fast / --cap-seed: playout cap randomisation in the self-play generation of `-m learn`.  CPU part:
the flags are listed, written to log/settings.txt, and a probability outside [0, 1] or a fast budget outside [-t, --mcts] is rejected.
GPU part: a learn iteration with the cap runs to its end and writes fewer samples than without, its samples are a function of
--cap-seed, and --cap-prob 1 is the run without the flags."""
import pytest

import host_cli as H
from host_cli import exe  # noqa: F401  (a fixture)

FLAGS = ("--cap-prob", "--cap-fast", "--cap-seed")


def test_help_and_settings_file_carry_the_flags(exe, tmp_path):
    H.check_flags_carried(exe, tmp_path, FLAGS, ("0.25", "20", "7"))


def test_the_defaults_are_off(exe, tmp_path):
    H.check_defaults(exe, tmp_path, FLAGS, ("1", "0", "0"))


@pytest.mark.parametrize("bad", ["-0.1", "1.5", "nan", "x", ""])
def test_a_value_that_is_no_probability_is_rejected(exe, tmp_path, bad):
    H.check_host_rejects(exe, tmp_path, ["--cap-prob=" + bad, "--cap-fast=2"], "--cap-prob")


@pytest.mark.parametrize("bad", ["1", "9", "-2", "x"])
def test_a_fast_budget_outside_threads_and_mcts_is_rejected(exe, tmp_path, bad):
    H.check_host_rejects(exe, tmp_path, ["--mcts=8", "-t", "2", "--cap-prob=0.5", "--cap-fast=" + bad], "--cap-fast")


@pytest.mark.parametrize("args,flag", [(["--cap-prob", "1.5", "--cap-fast", "2"], "--cap-prob"), (["--cap-prob", "nan", "--cap-fast", "2"], "--cap-prob"),
                                       (["--mcts", "8", "-t", "2", "--cap-prob", "0.5", "--cap-fast", "9"], "--cap-fast"),
                                       (["--mcts", "8", "-t", "2", "--cap-prob", "0.5", "--cap-fast", "1"], "--cap-fast")])
def test_learn_py_rejects_the_same_values(tmp_path, args, flag):
    H.check_learn_py_rejects(tmp_path, args, flag)


@pytest.fixture(scope="module")
def plain(exe, tmp_path_factory):
    """the run without the flags, shared"""
    return H.learn_records(exe, tmp_path_factory.mktemp("plain") / "run").raw


@pytest.mark.gpu
def test_learn_with_a_cap_writes_fewer_samples_as_a_function_of_cap_seed(exe, tmp_path, plain):
    a = H.learn_records(exe, tmp_path / "a", "--cap-prob", "0.5", "--cap-fast", "2", "--cap-seed", "7").raw
    b = H.learn_records(exe, tmp_path / "b", "--cap-prob", "0.5", "--cap-fast", "2", "--cap-seed", "7").raw
    c = H.learn_records(exe, tmp_path / "c", "--cap-prob", "0.5", "--cap-fast", "2", "--cap-seed", "8").raw
    assert len(a) < len(plain)
    assert a == b
    assert a != c


@pytest.mark.gpu
def test_cap_prob_one_is_the_run_without_the_flags(exe, tmp_path, plain):
    off = H.learn_records(exe, tmp_path / "off", "--cap-prob", "1", "--cap-fast", "2", "--cap-seed", "7").raw
    assert off == plain
