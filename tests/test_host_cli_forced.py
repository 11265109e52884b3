"""The C++ host's and learn.py's --forced-k / --prune-target: forced playouts and policy target pruning in the self-play generation of
`-m learn`.  CPU part: the flags are listed, written to log/settings.txt, off by default, and a factor outside [0, 8], a switch that
is neither 0 nor 1, or pruning without forcing is rejected.  GPU part: a learn iteration with both runs to its end; pruning changes the
policies of the samples and nothing else."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from gpu_common import ROOT

HOST = os.path.join(ROOT, "alphazero-risk_amd", "host")
EXE = os.path.join(HOST, "AlphaZero_Risk_hip")
FLAGS = ("--forced-k", "--prune-target")


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "alphazero-risk_amd", "csrc")])
    subprocess.check_call(["make", "-s", "-C", HOST])
    return EXE


def _settings(exe, path, *extra):
    # the settings file is written before the first engine is created: it exists whether or not the run finds a device
    subprocess.run([exe, "-m", "play", "--p1", "sp", "--p2", "rp", "--cg", "2", "--gpu-games", "2", *extra], cwd=path, capture_output=True,
                   text=True, timeout=600)
    return open(path / "log" / "settings.txt").read().splitlines()


def test_help_and_settings_file_carry_the_flags(exe, tmp_path):
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, check=True).stdout
    for flag in FLAGS:
        line = [l for l in out.split("\n") if l.strip().startswith(flag)]
        assert len(line) == 1 and "[this build]" in line[0], flag
    s = _settings(exe, tmp_path, "--forced-k", "2", "--prune-target", "1")
    for flag, value in zip(FLAGS, ("2", "1")):
        assert [l.rsplit(")=", 1)[1] for l in s if l.startswith(flag[2:] + "(")] == [value]


def test_the_defaults_are_off(exe, tmp_path):
    s = _settings(exe, tmp_path)
    for flag in FLAGS:
        assert [l.rsplit(")=", 1)[1] for l in s if l.startswith(flag[2:] + "(")] == ["0"]


@pytest.mark.parametrize("bad", ["-0.5", "8.5", "nan", "x", ""])
def test_a_value_that_is_no_factor_is_rejected(exe, tmp_path, bad):
    r = subprocess.run([exe, "-m", "learn", "--forced-k=" + bad], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2 and "--forced-k" in r.stderr


@pytest.mark.parametrize("args", [["--forced-k=2", "--prune-target=2"], ["--forced-k=2", "--prune-target=x"], ["--prune-target=1"],
                                  ["--forced-k=0", "--prune-target=1"]])
def test_a_bad_switch_or_pruning_without_forcing_is_rejected(exe, tmp_path, args):
    r = subprocess.run([exe, "-m", "learn", *args], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2 and "--prune-target" in r.stderr


@pytest.mark.parametrize("args,flag", [(["--forced-k", "8.5"], "--forced-k"), (["--forced-k", "nan"], "--forced-k"),
                                       (["--forced-k", "-1"], "--forced-k"), (["--prune-target", "1"], "--prune-target"),
                                       (["--forced-k", "2", "--prune-target", "2"], "--prune-target")])
def test_learn_py_rejects_the_same_values(tmp_path, args, flag):
    """learn.py checks its arguments before it creates an engine: no device needed"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "alphazero-risk_amd", "learn.py"), *args], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2 and flag in r.stderr.splitlines()[-1]


def test_learn_py_lists_the_flags():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "alphazero-risk_amd", "learn.py"), "--help"], capture_output=True, text=True, check=True).stdout
    for flag in FLAGS:
        assert flag in out
    assert out.count("[this build] self-play forced playouts") == 1 and out.count("[this build] self-play policy target pruning") == 1


def _learn(exe, path, *extra):
    """one learn iteration; the records of its self-play games [n, 265].  data/training_samples.bin holds them first, in the order
    they were generated, and behind them the records of the compare games, which the freshly trained net plays and which therefore
    depend on every byte of the self-play records"""
    os.makedirs(path)
    r = subprocess.run([exe, "-m", "learn", "--mcts=8", "--gpu-games=16", "--blocks=1", "--ti=1", "--tg=2", "--dtype=bf16",
                        "--bs=64", "-e", "1", "--cg=2", "--ct=0", *extra],
                       cwd=path, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr + r.stdout[-2000:]
    assert "Self-play: 2 games" in r.stdout and "Erased" not in r.stdout
    n = int(re.search(r"Generated (\d+) new samples for total (\d+)", r.stdout).group(1))
    raw = open(os.path.join(path, "data", "training_samples.bin"), "rb").read()
    assert n > 0 and len(raw) >= 8 + 265 * n and (len(raw) - 8) % 265 == 0
    return np.frombuffer(raw[8:8 + 265 * n], np.uint8).reshape(n, 265)


@pytest.mark.gpu
def test_learn_with_forcing_and_pruning(exe, tmp_path):
    plain = _learn(exe, tmp_path / "plain")
    forced = _learn(exe, tmp_path / "forced", "--forced-k", "2")
    pruned = _learn(exe, tmp_path / "pruned", "--forced-k", "2", "--prune-target", "1")
    assert forced.shape != plain.shape or (forced != plain).any()      # forcing changes the search, so the games
    # pruning keeps the games: the same self-play records outside pi (bytes 93..264)
    assert pruned.shape == forced.shape
    assert (forced[:, :93] == pruned[:, :93]).all() and (forced[:, 93:] != pruned[:, 93:]).any()
