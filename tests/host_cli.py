"""Shared by the tests of the C++ host's command line (tests/test_host_cli*.py): the binary, built once; the settings file a command
line writes; what every self-play option's file asserts about its flags; one learn iteration and the records it leaves."""
import collections
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from gpu_common import ROOT

HOST = os.path.join(ROOT, "alphazero-risk_amd", "host")
LEARN = os.path.join(ROOT, "alphazero-risk_amd", "learn.py")


@functools.lru_cache(maxsize=None)
def built_exe():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "alphazero-risk_amd", "csrc")])
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "AlphaZero_Risk_hip")


@pytest.fixture(scope="module")
def exe():
    """the host binary (a test module imports this fixture by name)"""
    return built_exe()


def _settings(exe, path, *extra):
    """the lines of log/settings.txt under `path` after a run with the flags `extra`.  The file is written before the first engine is
    created: it exists whether or not the run finds a device"""
    subprocess.run([exe, "-m", "play", "--p1", "sp", "--p2", "rp", "--cg", "2", "--gpu-games", "2", *extra], cwd=path, capture_output=True,
                   text=True, timeout=600)
    return open(os.path.join(path, "log", "settings.txt")).read().splitlines()


def setting_values(lines, flags):
    """per flag, the values of its lines in a settings file (one line each, so one value each)"""
    return [[l.rsplit(")=", 1)[1] for l in lines if l.startswith(f[2:] + "(")] for f in flags]


# ---- what every self-play option's file asserts about its flags without a device ----------------------------------------------------
def check_flags_carried(exe, path, flags, values):
    """--help lists each flag once, marked "[this build]"; given `values`, log/settings.txt carries them"""
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, check=True).stdout
    for f in flags:
        line = [l for l in out.split("\n") if l.strip().split(" ")[0] == f]
        assert len(line) == 1 and "[this build]" in line[0], f
    given = [x for fv in zip(flags, values) for x in fv]
    assert setting_values(_settings(exe, path, *given), flags) == [[v] for v in values]


def check_defaults(exe, path, flags, values):
    assert setting_values(_settings(exe, path), flags) == [[v] for v in values]


def check_host_rejects(exe, path, args, flag):
    """`-m learn` with `args` ends with exit code 2 and a message that names the flag"""
    r = subprocess.run([exe, "-m", "learn", *args], cwd=path, capture_output=True, text=True)
    assert r.returncode == 2 and flag + ":" in r.stderr


def check_learn_py_rejects(path, args, flag, why=""):
    """learn.py checks its arguments before it creates an engine: no device needed.  The message is the range check's own (an argparse
    that does not know the flag exits with 2 as well)"""
    r = subprocess.run([sys.executable, LEARN, *args], cwd=path, capture_output=True, text=True)
    last = r.stderr.splitlines()[-1]
    assert r.returncode == 2 and flag + ":" in last and why in last, last


def check_learn_py_lists(flags, *phrases):
    """learn.py --help names the flags, and each phrase of their help texts once"""
    out = subprocess.run([sys.executable, LEARN, "--help"], capture_output=True, text=True, check=True).stdout
    assert all(f in out for f in flags) and all(out.count(p) == 1 for p in phrases)


LearnRun = collections.namedtuple("LearnRun", "records raw stdout")


def learn_records(exe, path, *extra, mcts=8, tg=2):
    """one learn iteration of `tg` self-play games in the new directory `path`: the records of its self-play games [n, 265], the bytes
    of data/training_samples.bin and the run's stdout.  The file holds the self-play records first, in the order they were generated,
    and behind them the records of the compare games, which the freshly trained net plays and which therefore depend on every byte of
    the self-play records"""
    os.makedirs(path, exist_ok=True)
    r = subprocess.run([exe, "-m", "learn", f"--mcts={mcts}", "--gpu-games=16", "--blocks=1", "--ti=1", f"--tg={tg}", "--dtype=bf16",
                        "--bs=64", "-e", "1", "--cg=2", "--ct=0", *extra],
                       cwd=path, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr + r.stdout[-2000:]
    assert f"Self-play: {tg} games" in r.stdout and "Erased" not in r.stdout
    n = int(re.search(r"Generated (\d+) new samples for total (\d+)", r.stdout).group(1))
    raw = open(os.path.join(path, "data", "training_samples.bin"), "rb").read()
    assert n > 0 and len(raw) > 8 + 265 and len(raw) >= 8 + 265 * n and (len(raw) - 8) % 265 == 0
    return LearnRun(np.frombuffer(raw[8:8 + 265 * n], np.uint8).reshape(n, 265), raw, r.stdout)
