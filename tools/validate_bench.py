#!/usr/bin/env python3
"""Time the validation pass of `-m analysis` (azr_nn_validate: the step's forward and losses with batch norm on the moving
statistics, no update) next to the optimiser step (azr_nn_train) on the same handle, at the reference's training shape.
    python tools/validate_bench.py [--blocks 20] [--bs 512] [--batches 8] [--reps 3]
Prints one JSON line: ms per validation batch, validated records/s, ms per optimiser step, and their ratio.  Each figure is the
best of --reps calls of --batches batches (one call = all batches queued back to back, one read-back)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P = importlib.import_module("alphazero-risk_amd")


def records(n, seed):
    """synthetic records on arbitrary boards: the pass does the same work whatever the positions"""
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, 265), np.uint8)
    rec[:, 0] = rng.integers(0, 2, n)
    rec[:, 1:43] = rng.integers(0, 256, (n, 42))
    rec[:, 43] = rec[:, 0]
    pi = rng.uniform(0, 1, (n, 43)).astype(np.float32)
    pi /= pi.sum(1, keepdims=True)
    rec[:, 89:93] = rng.integers(-1, 2, n).astype(np.float32).view(np.uint8).reshape(n, 4)
    rec[:, 93:] = pi.view(np.uint8).reshape(n, 172)
    return rec


def best_ms(fn, reps):
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--bs", type=int, default=512)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    eng = P.Engine(8, blocks=a.blocks, sims=1, node_capacity=64)
    eng.init_random(20260002)
    rec = records(a.bs * a.batches, seed=1)
    eng.train(rec[:a.bs], 1, batch_size=a.bs, rng_state=1)        # warm-up: training context, kernels loaded
    eng.validate(rec[:a.bs], batch_size=a.bs)
    val_ms = best_ms(lambda: eng.validate(rec, batch_size=a.bs), a.reps) / a.batches
    step_ms = best_ms(lambda: eng.train(rec, 1, batch_size=a.bs, rng_state=1), a.reps) / a.batches
    print(json.dumps({"blocks": a.blocks, "batch_size": a.bs, "batches_per_call": a.batches,
                      "validate_ms_per_batch": round(val_ms, 3), "validate_records_per_s": round(a.bs / val_ms * 1e3),
                      "train_ms_per_step": round(step_ms, 3), "validate_over_step": round(val_ms / step_ms, 3)}))
    eng.close()


if __name__ == "__main__":
    main()
