"""The C++ host's and learn.py's --q-share: the value mix of the records in the self-play generation of `-m learn`.  CPU part: the flag
is listed, written to log/settings.txt, off by default, and a share outside [0, 1] is rejected with the option's name.  GPU part: a
learn iteration with the mix on runs to its end and writes a data file whose value targets are no longer all in {-1, 0, 1}."""
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
FLAG = "--q-share"


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "alphazero-risk_amd", "csrc")])
    subprocess.check_call(["make", "-s", "-C", HOST])
    return EXE


def _setting(exe, path, *extra):
    # the settings file is written before the first engine is created: it exists whether or not the run finds a device
    subprocess.run([exe, "-m", "play", "--p1", "sp", "--p2", "rp", "--cg", "2", "--gpu-games", "2", *extra], cwd=path, capture_output=True,
                   text=True, timeout=600)
    lines = open(path / "log" / "settings.txt").read().splitlines()
    return [l.rsplit(")=", 1)[1] for l in lines if l.startswith(FLAG[2:] + "(")]


def test_help_and_settings_file_carry_the_flag(exe, tmp_path):
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, check=True).stdout
    line = [l for l in out.split("\n") if l.strip().startswith(FLAG)]
    assert len(line) == 1 and "[this build]" in line[0]
    assert _setting(exe, tmp_path, FLAG, "0.25") == ["0.25"]


def test_the_default_is_off(exe, tmp_path):
    assert _setting(exe, tmp_path) == ["0"]


@pytest.mark.parametrize("arg", ["--q-share=-0.5", "--q-share=1.5", "--q-share=nan", "--q-share=x", "--q-share="])
def test_the_cli_rejects_a_bad_value(exe, tmp_path, arg):
    r = subprocess.run([exe, "-m", "learn", arg], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2 and FLAG in r.stderr


@pytest.mark.parametrize("value", ["-0.5", "1.5", "nan"])
def test_learn_py_rejects_the_same_values(tmp_path, value):
    """learn.py checks its arguments before it creates an engine: no device needed"""
    r = subprocess.run([sys.executable, LEARN, FLAG, value], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2 and FLAG in r.stderr.splitlines()[-1]


def test_learn_py_lists_the_flag():
    out = subprocess.run([sys.executable, LEARN, "--help"], capture_output=True, text=True, check=True).stdout
    assert FLAG in out and out.count("[this build] self-play value mix") == 1


@pytest.mark.gpu
def test_learn_with_the_value_mix(exe, tmp_path):
    r = subprocess.run([exe, "-m", "learn", "--mcts=8", "--gpu-games=16", "--blocks=1", "--ti=1", "--tg=2", "--dtype=bf16", "--bs=64", "-e", "1",
                        "--cg=2", "--ct=0", FLAG, "0.5"], cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr + r.stdout[-2000:]
    assert "Self-play: 2 games" in r.stdout and "Erased" not in r.stdout
    n = int(re.search(r"Generated (\d+) new samples for total (\d+)", r.stdout).group(1))
    raw = open(os.path.join(tmp_path, "data", "training_samples.bin"), "rb").read()
    assert n > 0 and len(raw) >= 8 + 265 * n and (len(raw) - 8) % 265 == 0
    z = np.frombuffer(raw[8:], np.uint8).reshape(-1, 265)[:, 89:93].copy().view(np.float32)[:, 0]
    assert (np.abs(z) <= 1).all() and (~np.isin(z, [-1.0, 0.0, 1.0])).any()
