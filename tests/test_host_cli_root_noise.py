"""The C++ host's --dir-alpha / --dir-seed: sampled root noise in the self-play generation of `-m learn`.  CPU part: the flags are
listed, written to log/settings.txt and a value that is no Dirichlet parameter is rejected.  GPU part: a learn iteration with noise
runs to its end, its samples are a function of --dir-seed, and --dir-alpha 0 is the run without the flags."""
import os
import subprocess

import pytest

from gpu_common import ROOT

HOST = os.path.join(ROOT, "alphazero-risk_amd", "host")
EXE = os.path.join(HOST, "AlphaZero_Risk_hip")


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "alphazero-risk_amd", "csrc")])
    subprocess.check_call(["make", "-s", "-C", HOST])
    return EXE


def test_help_and_settings_file_carry_the_flags(exe, tmp_path):
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, check=True).stdout
    for flag in ("--dir-alpha", "--dir-seed"):
        line = [l for l in out.split("\n") if l.strip().startswith(flag)]
        assert len(line) == 1 and "[this build]" in line[0], flag
    # the settings file is written before the first engine is created: it exists whether or not the run finds a device
    subprocess.run([exe, "-m", "play", "--p1", "sp", "--p2", "rp", "--cg", "2", "--gpu-games", "2", "--dir-alpha", "0.3", "--dir-seed", "7"],
                   cwd=tmp_path, capture_output=True, text=True, timeout=600)
    s = open(tmp_path / "log" / "settings.txt").read().splitlines()
    assert [l.rsplit(")=", 1)[1] for l in s if l.startswith("dir-alpha(")] == ["0.3"]
    assert [l.rsplit(")=", 1)[1] for l in s if l.startswith("dir-seed(")] == ["7"]


@pytest.mark.parametrize("bad", ["-1", "10.5", "nan", "x"])
def test_a_value_that_is_no_dirichlet_parameter_is_rejected(exe, tmp_path, bad):
    r = subprocess.run([exe, "-m", "learn", "--dir-alpha=" + bad], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2 and "--dir-alpha" in r.stderr


def _learn(exe, path, *extra):
    os.makedirs(path)
    r = subprocess.run([exe, "-m", "learn", "--mcts=8", "--gpu-games=16", "--blocks=1", "--ti=1", "--tg=2", "--dtype=bf16",
                        "--bs=64", "-e", "1", "--cg=2", "--ct=0", *extra],
                       cwd=path, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr + r.stdout[-2000:]
    assert "Self-play: 2 games" in r.stdout
    raw = open(os.path.join(path, "data", "training_samples.bin"), "rb").read()
    assert len(raw) > 8 + 265
    return raw


@pytest.mark.gpu
def test_learn_with_root_noise_is_a_function_of_dir_seed(exe, tmp_path):
    a = _learn(exe, tmp_path / "a", "--dir-alpha", "0.3", "--dir-seed", "7")
    b = _learn(exe, tmp_path / "b", "--dir-alpha", "0.3", "--dir-seed", "7")
    c = _learn(exe, tmp_path / "c", "--dir-alpha", "0.3", "--dir-seed", "8")
    assert a == b
    assert a != c


@pytest.mark.gpu
def test_dir_alpha_zero_is_the_run_without_the_flags(exe, tmp_path):
    off = _learn(exe, tmp_path / "off", "--dir-alpha", "0", "--dir-seed", "7")
    absent = _learn(exe, tmp_path / "absent")
    assert off == absent
