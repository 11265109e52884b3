"""The C++ host's and learn.py's --gumbel-m / --gumbel-cvisit / --gumbel-cscale / --gumbel-seed: the Gumbel root search in the
self-play generation of `-m learn`.  CPU part: the flags are listed, written to log/settings.txt, off by default, and a bad value is
rejected with the option's name.  GPU part: a learn iteration with the four flags runs to its end, says so in its log line, and writes
records whose pi is a softmax over the legal moves (no multiples of 1 / 16) — the flags reached the engine."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from gpu_common import ROOT

HOST = os.path.join(ROOT, "alphazero-risk_amd", "host")
EXE = os.path.join(HOST, "AlphaZero_Risk_hip")
LEARN = os.path.join(ROOT, "alphazero-risk_amd", "learn.py")
FLAGS = ("--gumbel-m", "--gumbel-cvisit", "--gumbel-cscale", "--gumbel-seed")


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "alphazero-risk_amd", "csrc")])
    subprocess.check_call(["make", "-s", "-C", HOST])
    return EXE


def _settings(exe, path, *extra):
    # the settings file is written before the first engine is created: it exists whether or not the run finds a device
    subprocess.run([exe, "-m", "play", "--p1", "sp", "--p2", "rp", "--cg", "2", "--gpu-games", "2", *extra], cwd=path, capture_output=True,
                   text=True, timeout=600)
    lines = open(path / "log" / "settings.txt").read().splitlines()
    return [[l.rsplit(")=", 1)[1] for l in lines if l.startswith(f[2:] + "(")] for f in FLAGS]


def test_help_and_settings_file_carry_the_flags(exe, tmp_path):
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, check=True).stdout
    for f in FLAGS:
        line = [l for l in out.split("\n") if l.strip().split(" ")[0] == f]
        assert len(line) == 1 and "[this build]" in line[0], f
    assert _settings(exe, tmp_path, "--gumbel-m", "8", "--gumbel-cvisit", "40", "--gumbel-cscale", "0.25", "--gumbel-seed", "9") == [["8"], ["40"], ["0.25"], ["9"]]


def test_the_default_is_off(exe, tmp_path):
    assert _settings(exe, tmp_path) == [["0"], ["50"], ["0.5"], ["0"]]


@pytest.mark.parametrize("arg", ["--gumbel-m=44", "--gumbel-m=-1", "--gumbel-m=x", "--gumbel-m=", "--gumbel-cvisit=-1", "--gumbel-cvisit=nan",
                                 "--gumbel-cscale=0", "--gumbel-cscale=inf", "--gumbel-cscale=x", "--gumbel-seed=-1", "--gumbel-seed=4294967296"])
def test_the_cli_rejects_a_bad_value(exe, tmp_path, arg):
    r = subprocess.run([exe, "-m", "learn", arg], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2 and arg.split("=")[0] in r.stderr


@pytest.mark.parametrize("args,why", [(("--gumbel-m", "44"), "is not a number of root moves"), (("--gumbel-cvisit", "-1"), "is not a c_visit"),
                                      (("--gumbel-cscale", "0"), "is not a c_scale"), (("--gumbel-cscale", "nan"), "is not a c_scale"),
                                      (("--gumbel-seed", "-1"), "is not a 32-bit seed"),
                                      (("--gumbel-m", "4", "--dir-alpha", "0.3"), "does not go with --dir-alpha")])
def test_learn_py_rejects_the_same_values(tmp_path, args, why):
    """learn.py checks its arguments before it creates an engine: no device needed.  The message is the range check's own (an argparse
    that does not know the flag exits with 2 as well)"""
    r = subprocess.run([sys.executable, LEARN, *args], cwd=tmp_path, capture_output=True, text=True)
    last = r.stderr.splitlines()[-1]
    assert r.returncode == 2 and args[0] in last and why in last, last


def test_learn_py_lists_the_flags():
    out = subprocess.run([sys.executable, LEARN, "--help"], capture_output=True, text=True, check=True).stdout
    assert all(f in out for f in FLAGS) and out.count("[this build] self-play Gumbel root search") == 1


@pytest.mark.gpu
def test_learn_with_the_gumbel_search(exe, tmp_path):
    r = subprocess.run([exe, "-m", "learn", "--mcts=16", "--gpu-games=16", "--blocks=1", "--ti=1", "--tg=2", "--dtype=bf16", "--bs=64", "-e", "1",
                        "--cg=2", "--ct=0", "--gumbel-m", "4", "--gumbel-cvisit", "50", "--gumbel-cscale", "0.5", "--gumbel-seed", "9"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr + r.stdout[-2000:]
    assert "Self-play: 2 games" in r.stdout and "Erased" not in r.stdout
    assert "Gumbel root search: m 4, c_visit 50, c_scale 0.5, seed 9" in r.stdout
    n = int(re.search(r"Generated (\d+) new samples for total (\d+)", r.stdout).group(1))
    raw = open(os.path.join(tmp_path, "data", "training_samples.bin"), "rb").read()
    assert n > 0 and len(raw) >= 8 + 265 * n and (len(raw) - 8) % 265 == 0
    pi = np.frombuffer(raw[8:], np.uint8).reshape(-1, 265)[:, 93:265].copy().view(np.float32)
    assert np.abs(pi.astype(np.float64).sum(1) - 1).max() <= 43 * 2.0 ** -24
    # the entries of a visit distribution over 16 simulations are multiples of 1/16; a softmax's are not
    assert (np.abs(pi * 16 - np.rint(pi * 16)) > 1e-3).any()
