"""Policy surprise weighting of the self-play records, restated from include/azr.h in np.float32, operation for operation (TEST
INFRASTRUCTURE): the engine's logarithm, a record's surprise KL(pi || P), a finished game's weights, and the coin that rounds a weight
to a copy count.  Every float operation below is one fp32 operation of the header, rounded on its own; integers are Python's, masked
to 32 bits.

tests/test_surprise_ref.py checks the restatement against float64 on the CPU; tests/test_gpu_surprise_weighting.py pins the device to
it bit for bit."""
import numpy as np

from azr_testlib import bits
from playout_cap_ref import M32, mix

f32 = np.float32
TINY = f32(1.17549435e-38)
MOVES = 43


def ln32(x):
    """the header's ln32, for a scalar or an array"""
    x = np.asarray(x, f32)
    x = np.where(x < TINY, TINY, x).astype(f32)
    b = x.view(np.uint32)
    e = (b >> np.uint32(23)).astype(np.int32) - 127
    m = ((b & np.uint32(0x7FFFFF)) | np.uint32(0x3F800000)).view(f32)
    big = m > f32(1.41421354)
    m = np.where(big, m * f32(0.5), m).astype(f32)
    e = e + big.astype(np.int32)
    t = (m - f32(1.0)) / (m + f32(1.0))
    t2 = t * t
    p = np.full(t.shape, 0.111111112, f32)
    for c in (0.142857149, 0.2, 0.333333343, 1.0):
        p = p * t2 + f32(c)
    out = e.astype(f32) * f32(0.693147182) + (f32(2.0) * t) * p
    assert out.dtype == f32
    return out


def record_kl(pi, prior, valid):
    """KL(pi || P) of one record: pi, prior float32 [43], valid the legal-move mask"""
    pi, prior = np.asarray(pi, f32), np.asarray(prior, f32)
    ok = bits(valid) & (pi > 0)
    term = np.where(ok, pi * (ln32(pi) - ln32(prior)), f32(0.0)).astype(f32)
    kl = f32(0.0)
    for m in range(MOVES):
        kl = f32(kl + term[m])
    return kl if kl > 0 else f32(0.0)


def game_weights(kl, share, max_weight):
    """w_r of a finished game's records from their surprises in staging order"""
    kl = np.asarray(kl, f32)
    n = len(kl)
    S = f32(0.0)
    for v in kl:
        S = f32(S + v)
    if not S > 0:
        return np.ones(n, f32)
    share, max_weight = f32(share), f32(max_weight)
    w = (f32(1.0) - share) + (share * f32(n)) * (kl / S)
    assert w.dtype == f32
    return np.minimum(w, max_weight)


def copies(w, seed, game_seed, r):
    """c_r of record r with weight w"""
    w = f32(w)
    base = int(w)
    thr = int(f32(w - f32(base)) * f32(16777216.0))
    k = mix(seed + 0x165667B1)
    k = mix(k ^ (game_seed & M32))
    k = mix(((k ^ (r & M32)) + 0xD3A2646C) & M32)
    return base + int((k >> 8) < thr)


def game_copies(kl, share, max_weight, seed, game_seed):
    """(w [n] float32, c [n] uint32) of one finished game"""
    w = game_weights(kl, share, max_weight)
    return w, np.array([copies(w[r], seed, game_seed, r) for r in range(len(w))], np.uint32)
