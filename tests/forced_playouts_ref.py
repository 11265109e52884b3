"""Forced playouts and policy target pruning at the root, restated from include/azr.h in np.float32 (TEST INFRASTRUCTURE).

Every operation is one fp32 operation on np.float32 operands, in the order the header writes them, so each is rounded on its own as
the device's __fmul_rn / __fadd_rn / sqrtf / __fdiv_rn are.  puct_pick is tree_select's root-level selection with a root vector
(the restatement tests/test_gpu_root_noise.py checks against the device); forced_pick is the same selection run over the forced moves
alone where there are any; prune_counts is the header's loop; root_policy is calculateMoveProbability(1.0f)."""
import numpy as np

from azr_testlib import bits

f32 = np.float32
MOVES = 43


def umap_order(orc, valid):
    """the moves of `valid` in the reference's unordered_map iteration order (the oracle's orc_umap_order)"""
    import azr_testlib as T
    order = np.zeros(MOVES, np.uint8)
    k = orc.orc_umap_order(int(valid), T.ptr(order))
    return [int(m) for m in order[:k]]


def noised_prior(Pr, eta, eps):
    c1 = f32(1) - f32(eps)
    return (c1 * Pr.astype(f32)) + (f32(eps) * eta.astype(f32))


def scores(N, Q, noiseP, hp):
    """(u, v) of tree_select: v = (noiseP * hp) * sqrt(1 + sumN), u = Q + v / (1 + N)"""
    sumN = f32(int(N.sum()))
    v = (noiseP * f32(hp)) * np.sqrt(f32(1) + sumN)
    u = Q.astype(f32) + v / (f32(1) + N.astype(f32))
    assert u.dtype == f32 and v.dtype == f32
    return u, v


def forced_counts(N, noiseP, k):
    """nf[m] = sqrt((k * noiseP[m]) * (float)sumN); NaN where noiseP is negative"""
    sumN = f32(int(N.sum()))
    with np.errstate(invalid="ignore"):
        nf = np.sqrt((f32(k) * noiseP) * sumN)
    assert nf.dtype == f32
    return nf


def _first_max(u, cand, valid, order):
    """strict maximum of u over cand; ties in unordered_map order (order() is only asked when there is a tie)"""
    best = u[cand].max()
    ties = [m for m in range(MOVES) if cand[m] and u[m] == best]
    if len(ties) == 1:
        return ties[0]
    return [m for m in order() if m in ties][0]


def puct_pick(N, Q, Pr, valid, eta, eps, hp, order):
    """the root-level selection without forcing (one search thread: no move is in flight)"""
    ok = bits(valid)
    u, _ = scores(N, Q, noised_prior(Pr, eta, eps), hp)
    return _first_max(u, ok, valid, order)


def forced_mask(N, Pr, valid, eta, eps, k):
    ok = bits(valid)
    if not k > 0:
        return np.zeros(MOVES, bool)
    nf = forced_counts(N, noised_prior(Pr, eta, eps), k)
    with np.errstate(invalid="ignore"):
        return ok & (N > 0) & (N.astype(f32) < nf)


def forced_pick(N, Q, Pr, valid, eta, eps, hp, k, order):
    """the root-level selection with forced playouts of factor k: over the forced moves alone where there are any"""
    ok = bits(valid)
    u, _ = scores(N, Q, noised_prior(Pr, eta, eps), hp)
    forced = forced_mask(N, Pr, valid, eta, eps, k)
    return _first_max(u, forced if forced.any() else ok, valid, order)


def forced_cap(nf):
    """(uint32)nf truncated; 0 where nf is not a positive number"""
    return 0 if not nf > 0 else min(int(nf), (1 << 24) - 1)


def prune_counts(N, Q, Pr, valid, eta, eps, hp, k):
    """N' of policy target pruning: the header's loop, move by move"""
    ok = bits(valid)
    N = N.astype(np.int64)
    out = N.copy()
    if not ok.any():
        return out.astype(np.uint32)
    noiseP = noised_prior(Pr, eta, eps)
    u, v = scores(N, Q, noiseP, hp)
    nf = forced_counts(N, noiseP, k)
    top = N[ok].max()
    cstar = [m for m in range(MOVES) if ok[m] and N[m] == top][0]
    ustar = u[cstar]
    for m in range(MOVES):
        if not ok[m] or m == cstar or N[m] == 0:
            continue
        f = forced_cap(nf[m])
        lower = N[m] - f if N[m] > f else 0
        n = int(N[m])
        while n > lower and f32(Q[m]) + v[m] / (f32(1) + f32(n - 1)) < ustar:
            n -= 1
        if n == 1 and n < N[m]:
            n = 0
        out[m] = n
    return out.astype(np.uint32)


def root_policy(N, valid):
    """calculateMoveProbability(1.0f): N over the sequential fp32 sum of the legal N, index order"""
    ok = bits(valid)
    prob = np.where(ok, N.astype(f32), f32(0)).astype(f32)
    s = f32(0)
    for m in range(MOVES):
        if ok[m]:
            s = f32(s + prob[m])
    with np.errstate(invalid="ignore", divide="ignore"):
        return (prob / s).astype(f32)
