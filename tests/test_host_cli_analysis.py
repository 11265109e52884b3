"""The C++ host's `-m analysis` (executeAnalysis, src/alphazero_risk.cpp:64-82; AlphaZeroNN::trainCrossValidation,
alphazero_nn.cpp:412-575).  CPU: the loud failures without a sample file or without a device.  GPU: the mode end to end on
self-play records, and fold 0 / epoch 0 replayed through the Python binding (split and shuffles restated by
tests/helpers/cv_split_probe.cpp)."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from gpu_common import ROOT, have_gpu, pkg
from host_cli import exe  # noqa: F401  (a fixture)

F = r"-?(?:\d+\.\d{6}|nan|inf)"


def test_analysis_fails_loudly_without_samples_or_device(exe, tmp_path):
    if have_gpu():
        pytest.skip("needs a box without a GPU (checks the loud failure)")
    r = subprocess.run([exe, "-m", "analysis", "--blocks", "1"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 1 and "no training sample file" in r.stderr, (r.returncode, r.stderr)
    learn = importlib.import_module("alphazero-risk_amd.learn")
    learn.save_training_samples(str(tmp_path / "data" / "training_samples.bin"), np.zeros((4, 265), np.uint8))
    r = subprocess.run([exe, "-m", "analysis", "--blocks", "1"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 1 and "no ROCm-capable device" in r.stderr, (r.returncode, r.stderr)


def selfplay_records(n):
    P = pkg()
    eng = P.Engine(32, blocks=1, sims=4, dtype=P.NET_BF16, max_game_rounds=12)
    eng.init_random(2)
    eng.selfplay_start(9)
    while eng.counters()["samples"] < n:
        eng.selfplay_run(64)
    rec = eng.drain()
    eng.close()
    return rec


@pytest.mark.gpu
def test_analysis_mode_end_to_end_and_replay(exe, tmp_path):
    learn = importlib.import_module("alphazero-risk_amd.learn")
    rec = selfplay_records(300)
    n, bs, k = len(rec), 32, 2
    learn.save_training_samples(str(tmp_path / "data" / "training_samples.bin"), rec)
    r = subprocess.run([exe, "-m", "analysis", "--blocks", "1", "--bs", str(bs), "--cvk", str(k), "-e", "1", "--cv-max-epochs", "2"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout[-2000:]
    # stdout grammar: the reference's lines, two folds of two epochs (EPOCHS = 1 but the model is still "learning": capped at 2)
    pats = [r"Started cross-validation training", r"Cross-validation step: \d+/\d+", r"EPOCH \d+",
            rf"Training Loss Policy {F} Value: {F}", rf"Validation Loss Policy {F} Value: {F}", r"=> Stopped training model is not learning"]
    lines = [l for l in r.stdout.split("\n") if any(re.fullmatch(p, l) for p in pats)]
    want = ["Started cross-validation training"]
    for vi in range(k):
        want.append(f"Cross-validation step: {vi}/{k}")
        for e in range(2):
            want += [f"EPOCH {e}", "T", "V"]
    assert len(lines) == len(want), r.stdout[-3000:]
    for got, w in zip(lines, want):
        assert got.startswith("Training Loss" if w == "T" else "Validation Loss" if w == "V" else w) and (w in "TV" or got == w), (got, w)
    for vi in range(k):
        for e in range(2):
            assert os.path.getsize(tmp_path / "checkpoints" / f"cross-validation-{vi}-{e} .bin") > 0
    log = open(tmp_path / "log" / "azr-nn-training-log.txt").read().split("\n")
    assert log[-1] == "" and len(log) == 2 * k + 1
    for l in log[:-1]:
        assert re.fullmatch(r"[^,\s]+,[^,\s]+,[^,\s]+,[^,\s]+", l), l
        [float(x) for x in l.split(",")]

    # replay fold 0 / epoch 0: fresh net (seed 20260002 + 0), the minibatches of the shuffled training set, the shuffled validation set
    probe = str(tmp_path / "cv_split_probe")
    subprocess.check_call(["g++", "-O1", "-o", probe, os.path.join(ROOT, "tests", "helpers", "cv_split_probe.cpp")])
    out = subprocess.check_output([probe, str(n), str(k), "1"]).decode().split("\n")
    tr, va = np.array(out[0].split(), int), np.array(out[1].split(), int)
    assert len(tr) + len(va) == n and len(va) == n // k - 1
    P = pkg()
    eng = P.Engine(8, blocks=1, sims=1, node_capacity=64)
    eng.init_random(20260002)
    lp = lv = np.float32(0)
    nb = len(tr) // bs
    for c in range(nb):
        l = eng.train_batch(rec[tr[c * bs:(c + 1) * bs]])
        lp += np.float32(l[0]); lv += np.float32(l[1])
    eng.save(str(tmp_path / "replay.bin"))
    assert (tmp_path / "replay.bin").read_bytes() == (tmp_path / "checkpoints" / "cross-validation-0-0 .bin").read_bytes()
    vlp, vlv = eng.validate(rec[va], batch_size=bs)
    t_line, v_line = lines[3], lines[4]
    assert t_line == "Training Loss Policy %f Value: %f" % (np.float32(lp / np.float32(nb)), np.float32(lv / np.float32(nb)))
    assert v_line == "Validation Loss Policy %f Value: %f" % (vlp, vlv)
    eng.close()
