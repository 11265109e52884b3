"""Gumbel root search with sequential halving, restated from include/azr.h in np.float32, operation for operation (TEST
INFRASTRUCTURE): the engine's exponential, the Gumbel draw, the considered-visit sequence, the completed Q with v_mix and sigma, the
root-level selection with its fallbacks, the record's policy and the move.  Every float operation below is one fp32 operation of the
header, rounded on its own; integers are Python's, masked to 32 bits.

tests/test_gumbel_ref.py checks the restatement against float64 and the hand examples on the CPU; tests/test_gpu_gumbel.py pins the
device to it bit for bit."""
import numpy as np

from azr_testlib import bits
from playout_cap_ref import M32, mix
from surprise_ref import TINY, ln32

f32 = np.float32
MOVES = 43
NONE = 43
EXP32_MIN = f32(-104.0)
# the measured maximum relative error of exp32 against the float64 exp over test_gumbel_ref's grid, where the result is a normal
# float (the header's figure), and the maximum absolute error in units of the smallest denormal below that
EXP32_REL = 9.84e-8
EXP32_DENORMAL_ULP = 0.775


def _pow2(k):
    """the float 2^k for -126 <= k <= 127, by its bits"""
    return ((np.asarray(k, np.int32) + 127).astype(np.uint32) << np.uint32(23)).view(f32)


def exp32(x):
    """the header's exp32 for arguments <= 0, a scalar or an array"""
    x = np.asarray(x, f32)
    zero = x < EXP32_MIN
    xs = np.where(zero, f32(0.0), x).astype(f32)
    kf = np.rint(xs * f32(1.44269502)).astype(f32)
    k = kf.astype(np.int32)
    r = (xs - kf * f32(0.693145752)) - kf * f32(1.42860682e-06)
    p = np.full(xs.shape, 1.98412701e-04, f32)
    for c in (1.38888892e-03, 8.33333377e-03, 4.16666679e-02, 1.66666672e-01, 0.5, 1.0, 1.0):
        p = p * r + f32(c)
    k1 = k >> 1
    out = (p * _pow2(k1)) * _pow2(k - k1)
    assert out.dtype == f32
    return np.where(zero, f32(0.0), out).astype(f32)


def u01(key):
    """the first noise_u01 of the stream `key`"""
    return f32((f32(mix(key) >> 9) + f32(0.5)) * f32(1.0 / 8388608.0))


def draw(seed, game_seed, decision, valid, greedy=False):
    """g [43] of the root with the legal moves `valid` at decision `decision` of the game with seed `game_seed`"""
    g = np.zeros(MOVES, f32)
    if greedy:
        return g
    key = mix(seed + 0xB5297A4D)
    key = mix(key ^ (game_seed & M32))
    key = mix(((key ^ (decision & M32)) + 0x1B56C4E9) & M32)
    ok = bits(valid)
    for a in range(MOVES):
        if ok[a]:
            u = u01(mix(key ^ (((a + 1) * 0x9E3779B9) & M32)))
            g[a] = -ln32(-ln32(u))
    return g


def considered_visit(m_eff, n, i):
    """cv(m_eff, n, i)"""
    if m_eff <= 1:
        return i
    L = (m_eff - 1).bit_length()
    k, base, pos = m_eff, 0, 0
    while True:
        e = max(1, n // (L * k))
        if i < pos + e * k:
            return base + (i - pos) // k
        pos += e * k
        base += e
        k = max(2, k // 2)


def logit(P):
    P = np.asarray(P, f32)
    return ln32(np.where(P < TINY, TINY, P).astype(f32))


def completed_q(N, Q, P, vhat, valid):
    """(q_hat [43], v_mix): N the node's completed visits"""
    N, Q, P, vhat = np.asarray(N, np.uint32), np.asarray(Q, f32), np.asarray(P, f32), f32(vhat)
    ok = bits(valid)
    seen = ok & (N > 0)
    total = int(N[ok].astype(np.int64).sum()) & M32
    wp, wq = f32(0.0), f32(0.0)
    for a in range(MOVES):
        wp = f32(wp + (P[a] if seen[a] else f32(0.0)))
        wq = f32(wq + (f32(P[a] * Q[a]) if seen[a] else f32(0.0)))
    v_mix = vhat
    if total > 0 and wp > 0:
        fn = f32(total)
        v_mix = f32(f32(vhat + f32(fn * f32(wq / wp))) / f32(f32(1.0) + fn))
    return np.where(seen, Q, v_mix).astype(f32), v_mix


def scores(N, Q, P, g, vhat, valid, c_visit, c_scale):
    """(g + logit + sigma, logit + sigma, q_hat), each [43]; junk on illegal lanes"""
    N = np.asarray(N, np.uint32)
    ok = bits(valid)
    qhat, _ = completed_q(N, Q, P, vhat, valid)
    top = int(N[ok].max()) if ok.any() else 0
    scale = f32(f32(f32(c_visit) + f32(top)) * f32(c_scale))
    sigma = (scale * qhat).astype(f32)
    lg = logit(P)
    return ((np.asarray(g, f32) + lg) + sigma).astype(f32), (lg + sigma).astype(f32), qhat


def _best(cand, score):
    """the candidate with the largest score, lowest index on ties; NONE where no candidate's score is a number"""
    s = np.where(cand, score, -np.inf)
    top = s.max()
    hit = np.nonzero(cand & (s == top) & (s > -np.inf))[0]
    return int(hit[0]) if len(hit) else NONE


def select(N, N0, act, Q, P, g, vhat, valid, i, m, n, c_visit, c_scale):
    """(move, cv) of the root-level selection with the claim index i"""
    N, N0, act = np.asarray(N, np.int64), np.asarray(N0, np.int64), np.asarray(act, np.int64)
    ok = bits(valid)
    m_eff = min(m, int(ok.sum()))
    cv = considered_visit(m_eff, n, i)
    cnt = np.where(N > N0, N - N0, 0) + act
    cand = ok & (cnt == cv)
    if not cand.any():
        below = ok & (cnt < cv)
        if below.any():
            cand = below & (cnt == cnt[below].max())
    if not cand.any():
        cand = ok
    score, _, _ = scores(N.astype(np.uint32), Q, P, g, vhat, valid, c_visit, c_scale)
    return _best(cand, score), cv


def policy(N, Q, P, vhat, valid, c_visit, c_scale):
    """(pi [43], q_hat [43]) of the record"""
    ok = bits(valid)
    _, x, qhat = scores(N, Q, P, np.zeros(MOVES, f32), vhat, valid, c_visit, c_scale)
    pi = np.zeros(MOVES, f32)
    if not ok.any():
        return pi, qhat
    mx = x[ok].max()
    e = np.where(ok, exp32(np.where(ok, x - mx, f32(0.0)).astype(f32)), f32(0.0)).astype(f32)
    s = f32(0.0)
    for a in range(MOVES):
        s = f32(s + e[a])
    pi = np.where(ok, e / s, f32(0.0)).astype(f32)
    return pi, np.where(ok, qhat, f32(0.0)).astype(f32)


def move(N, N0, Q, P, g, vhat, valid, c_visit, c_scale):
    """the decision's move"""
    N, N0 = np.asarray(N, np.int64), np.asarray(N0, np.int64)
    ok = bits(valid)
    if not ok.any():
        return NONE
    ns = np.where(N > N0, N - N0, 0)
    score, _, _ = scores(N.astype(np.uint32), Q, P, g, vhat, valid, c_visit, c_scale)
    return _best(ok & (ns == ns[ok].max()), score)
