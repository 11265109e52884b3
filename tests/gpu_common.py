"""shared helpers for the -m gpu tests (they call the product only through the C-ABI binding)."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pkg():
    return importlib.import_module("alphazero-risk_amd")


def have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


# ---- arena helpers shared by the arena, scripted-samples and dropped-game tests -----------------------------------------------------
def run_arena(eng, k0, k1, total, cap, mirror, base):
    eng.arena_start(k0, k1, total, per_slot_cap=cap, mirror=mirror, base_seed=base)
    for _ in range(2000):
        if eng.arena_run(64):
            break
    else:
        raise AssertionError("arena did not finish")
    return eng.arena_results(), eng.arena_log()


def half_slot(g, G, base):
    """slot g of a G-slot concurrent arena = (half, first pair seed, pair stride) of tests/azr_testlib.orc_play_half_games"""
    return g & 1, base + (g >> 1), G // 2


def arena_play(eng, k0, k1, total, cap, mirror, base, script=False, az=False, chunk=None, sink=None):
    """the whole arena, draining after every run (in pieces of `chunk` records, each handed to `sink` instead of kept when
    given); returns (results, log, records, runs that came back unfinished)"""
    eng.arena_collect_scripted_samples(script)
    eng.arena_collect_samples(az)
    eng.arena_start(k0, k1, total, per_slot_cap=cap, mirror=mirror, base_seed=base)
    out, waits = [], 0
    for _ in range(2000):
        fin = eng.arena_run(64)
        if script or az:
            while True:
                r = eng.drain(chunk) if chunk else eng.drain()
                if len(r):
                    if sink:
                        sink(r)
                    else:
                        out.append(r)
                if not chunk or len(r) < chunk:
                    break
        if fin:
            break
        waits += 1
    else:
        raise AssertionError("arena did not finish")
    rec = np.concatenate(out) if out else np.zeros((0, 265), np.uint8)
    return eng.arena_results(), eng.arena_log(), rec, waits


def pi_of(rec):
    return rec[:, 93:265].copy().view(np.float32)


def assert_one_hot(rec):
    pi = pi_of(rec)
    assert ((pi == 1.0).sum(1) == 1).all() and ((pi != 0.0).sum(1) == 1).all()
