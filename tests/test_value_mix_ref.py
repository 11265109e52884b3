"""CPU: tests/value_mix_ref.py — the value mix of include/azr.h restated in np.float32 — against the same formulas in float64.

The bound, from the operation count (u = 2^-24, the unit roundoff of fp32; |Q[m]| <= 1, so A = sum N|Q| / sum N <= 1; first order in u,
the higher orders are below 1e-5 of it):
  * (float)N[m] is exact (N < 2^24).  A term N[m] * Q[m] is rounded once and then passes through at most 42 rounded additions (the
    first addition, to 0.0f, is exact), each with an error of at most u times a partial sum, and every partial sum is at most sum N|Q|
    in magnitude: |num - NUM| <= 43 u sum N|Q|.
  * den adds integers.  While sum N < 2^24 — any search: the sum is at most its simulations — every partial sum is an integer below 2^24
    and den is EXACT.  Past that each of its 42 additions may round: |den - DEN| <= 42 u DEN.
  * the division rounds once, and clamping to [-1, 1] moves q towards the true value, which lies there:
        |q - q64| <= 43 u A + u |q64| <= 44 u        with den exact,        <= 44 u + 42 u |q64| <= 86 u    where den rounds.
  * the blend: a = 1 - q_share rounds once (error <= u a), a * z is exact for z in {-1, 0, 1}, q_share * q rounds once (<= u), the
    addition rounds once (<= u |z'| <= u), and the error of q enters times q_share <= 1; the final clamp again moves towards the truth:
        |z' - z64| <= 44 u + 3 u = 47 u              with den exact,        <= 89 u                          where den rounds.
So: 43 multiply-add pairs, one divide, three blend roundings — 47 u, asserted as 48 u (below 50 * 2^-24) to cover the higher-order terms,
on every row a search can produce; 90 u on the rows whose N sum past 2^24, which only a debug call can hand in."""
import numpy as np
import pytest

import value_mix_ref as V

f32 = np.float32
U = 2.0 ** -24
ALL = (1 << 43) - 1
SHARES = (0.25, 0.3, 0.7, 1.0, 1.0 - 2.0 ** -24)


def _z64(q_share, N, Q, valid, z):
    """(q, z') in float64 from the same float32 inputs"""
    ok = V.bits(valid) & (np.asarray(N) > 0)
    n = np.asarray(N, np.float64)[ok]
    if n.sum() == 0:
        return 0.0, float(z)
    q = float((n * np.asarray(Q, np.float64)[ok]).sum() / n.sum())
    s = float(f32(q_share))
    return q, (1.0 - s) * float(z) + s * q


def _rows(seed, rows, nmax):
    rng = np.random.default_rng(seed)
    N = rng.integers(0, nmax, (rows, 43)).astype(np.uint32)
    N[rng.random((rows, 43)) < 0.3] = 0
    Q = rng.uniform(-1, 1, (rows, 43)).astype(f32)
    Q[rng.random((rows, 43)) < 0.1] = f32(1.0)
    Q[rng.random((rows, 43)) < 0.1] = f32(-1.0)
    valid = np.array([sum(1 << m for m in range(43) if rng.random() < 0.6) or 1 for _ in range(rows)], np.uint64)
    valid[::5] = ALL
    z = rng.choice(np.array([-1, 0, 1], f32), rows)
    return N, Q, valid, z


@pytest.mark.parametrize("nmax,bound", [(50, 48 * U), (300000, 48 * U), (1 << 24, 90 * U)])
def test_the_restatement_is_within_the_derived_bound_of_float64(nmax, bound):
    N, Q, valid, z = _rows(5 + nmax, 400, nmax)
    if bound < 50 * U:                                                # den exact: the premise of the 47 u
        assert int(N.astype(np.int64).sum(1).max()) < 1 << 24
    else:
        assert int(N.astype(np.int64).sum(1).max()) > 1 << 26
    worst = 0.0
    for share in SHARES:
        q, has, zz = V.mix_rows(share, N, Q, valid, z)
        for i in range(len(z)):
            q64, z64 = _z64(share, N[i], Q[i], valid[i], z[i])
            assert abs(float(q[i]) - q64) <= bound and abs(float(zz[i]) - z64) <= bound, (share, i, q[i], q64, zz[i], z64)
            worst = max(worst, abs(float(zz[i]) - z64))
    print("worst |z' - z64| = %.2f u (bound %.0f u)" % (worst / U, bound / U))


def test_a_share_of_one_gives_q():
    N, Q, valid, z = _rows(11, 200, 1000)
    q, has, zz = V.mix_rows(1.0, N, Q, valid, z)
    assert has.all() and zz.tobytes() == q.tobytes()


def test_a_row_without_visits_gives_z():
    N, Q, valid, z = _rows(12, 60, 1000)
    N[:30] = 0                                                        # no visit at all
    for i in range(30, 60):                                           # visits under illegal moves only
        N[i][V.bits(valid[i])] = 0
    valid[30] = 1; N[30] = 7; N[30, 0] = 0
    for share in SHARES:
        q, has, zz = V.mix_rows(share, N, Q, valid, z)
        assert not has.any() and not q.any() and zz.tobytes() == z.tobytes()


def test_illegal_moves_do_not_count():
    N, Q, valid, z = _rows(13, 200, 1000)
    valid[::5] = valid[1::5]                                          # no row with every move legal
    want = V.mix_rows(0.7, N, Q, valid, z)
    rng = np.random.default_rng(14)
    N2, Q2 = N.copy(), Q.copy()
    for i in range(len(z)):
        bad = ~V.bits(valid[i])
        assert bad.any()
        N2[i][bad] = rng.integers(0, 1 << 32, bad.sum(), dtype=np.uint64).astype(np.uint32)
        Q2[i][bad] = rng.choice(np.array([np.nan, np.inf, -np.inf, 3e38, -7.5, 0.0], f32), bad.sum())
    got = V.mix_rows(0.7, N2, Q2, valid, z)
    for a, b in zip(want, got):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("share", [0.3, 0.7, 1.0 - 2.0 ** -24])
def test_the_blend_stays_within_one(share):
    N, Q, valid, z = _rows(15, 300, 1 << 24)
    side = np.where(Q[::3, :1] > 0, f32(1.0), f32(-1.0))
    Q[::3] = side                                                     # every third row: q = +1 or -1, where the sums round alike
    z[::3] = side[:, 0]                                               # ... with z on q's side
    z[::6] = -side[::2, 0]                                            # ... and, every other one, against it
    q, has, zz = V.mix_rows(share, N, Q, valid, z)
    assert (np.abs(q[::3]) == 1).all()
    assert (np.abs(zz) <= 1).all() and (np.abs(q) <= 1).all() and np.isfinite(zz).all()
    assert (np.abs(zz) == 1).any()
