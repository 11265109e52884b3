"""shared helpers for the -m gpu tests (they call the product only through the C-ABI binding)."""
import importlib
import os
import sys

import numpy as np

import azr_testlib as T

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


# ---- the host-stepped search of the root-noise and forced-playouts tests --------------------------------------------------------------
def setup_engine(sims):
    P = pkg()
    eng = P.Engine(8, blocks=1, sims=sims, dtype=P.NET_F32, threads=1)
    eng.set_weights(T.make_net_flat(1, seed=23, perturb_bn=True))
    eng.new_games(np.arange(4100, 4108, dtype=np.uint32))   # setup phase: no descent of 24 ends in a finished game
    return eng


def stepped(eng, eta, passes, check):
    """begin / leaves / azr_nn_predict / apply one pass at a time; check(prev stats, new stats) between consecutive passes"""
    eng.set_root_noise(eta)
    eng.mcts_begin()
    x, need, act = eng.mcts_leaves()          # setRootState's root expansion
    eng.mcts_apply(*eng.predict(x))
    x, need, act = eng.mcts_leaves()          # the root is in the tree, descent 1 waits for the net
    prev = eng.root_stats()
    assert (prev[0] == 0).all()
    for i in range(passes):
        assert act == eng.G
        eng.mcts_apply(*eng.predict(x))
        x, need, act = eng.mcts_leaves()
        cur = eng.root_stats()
        check(i, prev, cur)
        prev = cur
    return prev


def pi_of(rec):
    return rec[:, 93:265].copy().view(np.float32)


def assert_one_hot(rec):
    pi = pi_of(rec)
    assert ((pi == 1.0).sum(1) == 1).all() and ((pi != 0.0).sum(1) == 1).all()


# ---- training records shared by the optimiser-step and validation tests -----------------------------------------------------------------
def records(n, seed=0):
    """synthetic (s, pi, z) records on real encoded positions: pi random over a random support, z in {-1, 0, 1}"""
    g = np.load(os.path.join(T.GOLDEN, "encode.npz"))
    x = g["in88"]
    rng = np.random.default_rng(seed)
    x = x[rng.integers(0, len(x), n)]
    pi = rng.uniform(0.0, 1.0, (n, 43)).astype(np.float32) * (rng.uniform(0, 1, (n, 43)) < 0.3)
    pi[:, 42] += 1e-3
    pi = (pi / pi.sum(1, keepdims=True)).astype(np.float32)
    z = rng.integers(-1, 2, n).astype(np.float32)
    rec = np.zeros((n, 265), np.uint8)
    rec[:, 0] = x[:, 42]
    rec[:, 1:89] = x
    rec[:, 89:93] = z.view(np.uint8).reshape(n, 4)
    rec[:, 93:265] = pi.view(np.uint8).reshape(n, 172)
    return rec
