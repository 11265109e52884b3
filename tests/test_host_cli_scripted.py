"""GPU: the C++ host's `-m train-data` (AlphaZeroTrainer::trainOnGeneratedData, alphazero_trainer.cpp:227-317) and
`-m train-script` (trainOnScript, :200-225) end to end — a net trained from the scripted players' recorded moves."""
import os
import re
import subprocess

import numpy as np
import pytest

from host_cli import exe  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu


def test_train_data_mode(exe, tmp_path):
    from log_grammar import GR, check
    common = ["-m", "train-data", "--dgss", "8", "--dgsr", "8", "--blocks", "1", "--bs", "64", "--cg", "4", "--ct", "0",
              "--gpu-games", "16"]
    r0 = subprocess.run([exe, *common, "--dtl", "0"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0, r0.stderr + r0.stdout[-2000:]
    start = open(tmp_path / "checkpoints" / "latest-checkpoint.bin", "rb").read()   # missing checkpoint => init + save
    r = subprocess.run([exe, *common, "--dtl", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr + r.stdout[-2000:]
    gen = [int(x) for x in re.findall(r"^Samples generated (\d+)$", r.stdout, re.M)]
    assert len(gen) == 2 and min(gen) > 8 * 100, r.stdout[-2000:]
    assert "EPOCH 2" in r.stdout and "Model improved" in r.stdout
    assert [len(x) for x in check("nn", open(tmp_path / "log" / "azr-nn-training-log.txt").read())] == [6]   # 3 epochs
    gr = re.compile(rf"^{GR}$")   # trainOnGeneratedData logs the bare GameResults (alphazero_trainer.cpp:297,309)
    for f in ("azr-improvement-log.txt", "azr-benchmark-log.txt"):
        lines = open(tmp_path / "log" / f).read().split("\n")
        assert lines[-1] == "" and len(lines) == 2 and gr.match(lines[0]), (f, lines)
    for f in ("checkpoint-data-epoch-0.bin", "latest-checkpoint.bin", "temp.bin"):
        assert os.path.getsize(tmp_path / "checkpoints" / f) > 0, f
    end = open(tmp_path / "checkpoints" / "latest-checkpoint.bin", "rb").read()
    assert len(end) == len(start) and end != start


def test_train_script_mode(exe, tmp_path):
    from log_grammar import GR, check
    r = subprocess.run([exe, "-m", "train-script", "--ti", "1", "--tg", "2", "--mcts", "8", "--blocks", "1", "--bs", "64",
                        "--cg", "2", "--ct", "0"], cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr + r.stdout[-2000:]
    assert "Started training on script player" in r.stdout and "Model improved" in r.stdout
    raw = open(tmp_path / "data" / "training_samples.bin", "rb").read()
    n = int(np.frombuffer(raw[:8], np.uint64)[0])
    assert n > 0 and len(raw) == 8 + n * 265
    rec = np.frombuffer(raw[8:], np.uint8).reshape(n, 265)
    nz = (rec[:, 93:].copy().view(np.float32).reshape(n, 43) != 0).sum(1)
    assert (nz == 1).any() and (nz > 1).any()   # the ScriptPlayer's one-hot moves and the AlphaZero player's visit distributions
    lines = open(tmp_path / "log" / "azr-benchmark-log.txt").read().split("\n")
    assert lines[-1] == "" and len(lines) == 2 and re.match(rf"^0,,,,{GR}$", lines[0]), lines   # alphazero_trainer.cpp:213
    assert len(check("improvement", open(tmp_path / "log" / "azr-improvement-log.txt").read())) == 1
