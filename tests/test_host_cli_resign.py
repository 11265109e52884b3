"""The C++ host's and learn.py's --resign-q, --resign-streak, --resign-holdout and --resign-seed: resignation with a no-resign holdout
in the self-play generation of `-m learn`.  CPU part: the flags are listed, written to log/settings.txt, off by default, and a value
outside its range is rejected with the option's name.  GPU part: a learn iteration with resignation on runs to its end, prints the
statistics line and writes a well-formed data file."""
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
FLAGS = ("--resign-q", "--resign-streak", "--resign-holdout", "--resign-seed")
STATS = r"Resignation: (\d+) resigned, (\d+) held out, (\d+) of them would have resigned, (\d+) of those did not lose  =>  false-positive share (\S+)"


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
    return {f: [l.rsplit(")=", 1)[1] for l in lines if l.startswith(f[2:] + "(")] for f in FLAGS}


def test_help_and_settings_file_carry_the_flags(exe, tmp_path):
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, check=True).stdout
    for flag in FLAGS:
        line = [l for l in out.split("\n") if l.strip().split(" ")[0] == flag]
        assert len(line) == 1 and "[this build]" in line[0], flag
    got = _settings(exe, tmp_path, "--resign-q", "-0.75", "--resign-streak", "3", "--resign-holdout", "0.25", "--resign-seed", "11")
    assert got == {"--resign-q": ["-0.75"], "--resign-streak": ["3"], "--resign-holdout": ["0.25"], "--resign-seed": ["11"]}


def test_the_default_is_off(exe, tmp_path):
    assert _settings(exe, tmp_path) == {"--resign-q": ["-0.9"], "--resign-streak": ["0"], "--resign-holdout": ["0.1"], "--resign-seed": ["0"]}


BAD = ["--resign-q=-1.5", "--resign-q=1.5", "--resign-q=nan", "--resign-q=x", "--resign-q=", "--resign-streak=-1", "--resign-streak=256",
       "--resign-streak=1.5", "--resign-streak=", "--resign-holdout=-0.1", "--resign-holdout=1.5", "--resign-holdout=nan",
       "--resign-seed=-1", "--resign-seed=4294967296", "--resign-seed=x"]


@pytest.mark.parametrize("arg", BAD)
def test_the_cli_rejects_a_bad_value(exe, tmp_path, arg):
    r = subprocess.run([exe, "-m", "learn", arg], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2 and arg.split("=")[0] + ":" in r.stderr


@pytest.mark.parametrize("flag,value", [("--resign-q", "-1.5"), ("--resign-q", "1.5"), ("--resign-q", "nan"), ("--resign-streak", "-1"),
                                        ("--resign-streak", "256"), ("--resign-holdout", "-0.1"), ("--resign-holdout", "1.5"),
                                        ("--resign-holdout", "nan"), ("--resign-seed", "-1"), ("--resign-seed", "4294967296")])
def test_learn_py_rejects_the_same_values(tmp_path, flag, value):
    """learn.py checks its arguments before it creates an engine: no device needed"""
    r = subprocess.run([sys.executable, LEARN, flag + "=" + value], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2 and flag + ":" in r.stderr.splitlines()[-1]


def test_learn_py_lists_the_flags():
    out = subprocess.run([sys.executable, LEARN, "--help"], capture_output=True, text=True, check=True).stdout
    assert all(f in out for f in FLAGS) and out.count("[this build] self-play resignation") == 1


@pytest.mark.gpu
def test_learn_with_resignation(exe, tmp_path):
    """every game held out, under the bound 1 that a root value of a running game lies below: all of them count, every one would have
    resigned at its first decision, and the false-positive share is that of the games the first mover did not lose"""
    r = subprocess.run([exe, "-m", "learn", "--mcts=8", "--gpu-games=16", "--blocks=1", "--ti=1", "--tg=4", "--dtype=bf16", "--bs=64", "-e", "1",
                        "--cg=2", "--ct=0", "--resign-q", "1", "--resign-streak", "1", "--resign-holdout", "1"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr + r.stdout[-2000:]
    assert "Self-play: 4 games" in r.stdout and "Erased" not in r.stdout
    m = re.search(STATS, r.stdout)
    assert m, r.stdout[-2000:]
    resigned, held, would, not_lost = (int(x) for x in m.groups()[:4])
    assert (resigned, held, would) == (0, 4, 4) and 0 <= not_lost <= 4 and float(m.group(5)) == not_lost / 4
    n = int(re.search(r"Generated (\d+) new samples for total (\d+)", r.stdout).group(1))
    raw = open(os.path.join(tmp_path, "data", "training_samples.bin"), "rb").read()
    assert n > 0 and len(raw) >= 8 + 265 * n and (len(raw) - 8) % 265 == 0
    z = np.frombuffer(raw[8:], np.uint8).reshape(-1, 265)[:, 89:93].copy().view(np.float32)[:, 0]
    assert set(z.tolist()) <= {-1.0, 0.0, 1.0}
