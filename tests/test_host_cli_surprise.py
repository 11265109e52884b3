"""The C++ host's and learn.py's --psw-share / --psw-max / --psw-seed: policy surprise weighting of the records in the self-play
generation of `-m learn`.  CPU part: the flags are listed, written to log/settings.txt, off by default, and a share outside [0, 1], a
cap outside [1, 64] or a seed that is no 32-bit number is rejected.  GPU part: a learn iteration with weighting on runs to its end and
writes a data file."""
import os
import re
import subprocess
import sys

import pytest

from gpu_common import ROOT

HOST = os.path.join(ROOT, "alphazero-risk_amd", "host")
EXE = os.path.join(HOST, "AlphaZero_Risk_hip")
LEARN = os.path.join(ROOT, "alphazero-risk_amd", "learn.py")
FLAGS = ("--psw-share", "--psw-max", "--psw-seed")


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


def _values(lines):
    return [[l.rsplit(")=", 1)[1] for l in lines if l.startswith(flag[2:] + "(")] for flag in FLAGS]


def test_help_and_settings_file_carry_the_flags(exe, tmp_path):
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, check=True).stdout
    for flag in FLAGS:
        line = [l for l in out.split("\n") if l.strip().startswith(flag)]
        assert len(line) == 1 and "[this build]" in line[0], flag
    assert _values(_settings(exe, tmp_path, "--psw-share", "0.5", "--psw-max", "8", "--psw-seed", "77")) == [["0.5"], ["8"], ["77"]]


def test_the_defaults_are_off(exe, tmp_path):
    assert _values(_settings(exe, tmp_path)) == [["0"], ["4"], ["0"]]


@pytest.mark.parametrize("arg", ["--psw-share=-0.5", "--psw-share=1.5", "--psw-share=nan", "--psw-share=x", "--psw-share=",
                                 "--psw-max=0.5", "--psw-max=65", "--psw-max=nan", "--psw-max=x", "--psw-max=",
                                 "--psw-seed=-1", "--psw-seed=4294967296", "--psw-seed=x", "--psw-seed="])
def test_the_cli_rejects_a_bad_value(exe, tmp_path, arg):
    r = subprocess.run([exe, "-m", "learn", arg], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2 and arg.split("=")[0] in r.stderr


@pytest.mark.parametrize("args", [["--psw-share", "-0.5"], ["--psw-share", "1.5"], ["--psw-share", "nan"], ["--psw-max", "0.5"],
                                  ["--psw-max", "65"], ["--psw-max", "nan"], ["--psw-seed", "-1"], ["--psw-seed", "4294967296"]])
def test_learn_py_rejects_the_same_values(tmp_path, args):
    """learn.py checks its arguments before it creates an engine: no device needed"""
    r = subprocess.run([sys.executable, LEARN, *args], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2 and args[0] in r.stderr.splitlines()[-1]


def test_learn_py_lists_the_flags():
    out = subprocess.run([sys.executable, LEARN, "--help"], capture_output=True, text=True, check=True).stdout
    for flag in FLAGS:
        assert flag in out
    assert out.count("[this build] self-play policy surprise weighting") == 1


@pytest.mark.gpu
def test_learn_with_surprise_weighting(exe, tmp_path):
    r = subprocess.run([exe, "-m", "learn", "--mcts=8", "--gpu-games=16", "--blocks=1", "--ti=1", "--tg=2", "--dtype=bf16", "--bs=64", "-e", "1",
                        "--cg=2", "--ct=0", "--psw-share", "0.5"], cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr + r.stdout[-2000:]
    assert "Self-play: 2 games" in r.stdout and "Erased" not in r.stdout
    n = int(re.search(r"Generated (\d+) new samples for total (\d+)", r.stdout).group(1))
    raw = open(os.path.join(tmp_path, "data", "training_samples.bin"), "rb").read()
    assert n > 0 and len(raw) >= 8 + 265 * n and (len(raw) - 8) % 265 == 0
