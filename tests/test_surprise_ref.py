"""CPU: tests/surprise_ref.py — the np.float32 restatement of policy surprise weighting (include/azr.h) — against float64, and the
statistics of its copy coin.  The bounds: the header's for ln32 (5e-7 relative, 1.6e-5 absolute: about 4 ulp, twice what the series
measures), 1e-5 absolute for a record's KL (measured: 1.2e-6), 1e-4 relative for a game's weight total, 6 standard errors for the
coin.  Every measured maximum is printed."""
import numpy as np

import playout_cap_ref as R
import surprise_ref as S

f32 = np.float32


def _ln_args():
    rng = np.random.default_rng(1)
    x = np.concatenate([
        np.exp(rng.uniform(np.log(1e-38), np.log(2.0), 1_000_000)),       # every binade of (1e-38, 2]
        rng.uniform(0.5, 2.0, 600_000),                                   # around 1, where ln x is small
        1.0 + rng.uniform(-2e-3, 2e-3, 200_000),
        np.array([1.0, 2.0, 0.5, 1.41421354, 1.41421366, 0.70710677, 1.17549435e-38, 1e-38 * 1.0000001]),
    ]).astype(f32)
    return x[(x > f32(1e-38)) & (x <= f32(2.0))]


def test_ln32_against_the_float64_logarithm():
    x = _ln_args()
    got = S.ln32(x).astype(np.float64)
    want = np.log(np.maximum(x, S.TINY).astype(np.float64))
    err = np.abs(got - want)
    big = np.abs(want) > 1e-3
    rel = (err[big] / np.abs(want[big])).max()
    print("ln32 over %d arguments: max relative error %.3g where |ln x| > 1e-3, max absolute error %.3g" % (len(x), rel, err.max()))
    assert rel <= 5e-7
    assert err.max() <= 1.6e-5
    assert S.ln32(f32(1.0)) == 0.0 and S.ln32(f32(1.0)).tobytes() == f32(0.0).tobytes()
    # zero and subnormals count as the smallest normal float
    tiny = S.ln32(S.TINY)
    assert S.ln32(f32(0.0)) == tiny and S.ln32(f32(1e-45)) == tiny and S.ln32(f32(5e-39)) == tiny and abs(float(tiny) + 87.3365) < 1e-3


def _pairs(n, seed):
    """(pi from 100 multinomial visits, Dirichlet(0.3) P, legal mask) — pi puts weight on legal moves only"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ok = np.ones(43, bool) if i % 2 == 0 else rng.random(43) < 0.4
        if not ok.any():
            ok[int(rng.integers(43))] = True
        P = np.zeros(43)
        P[ok] = rng.dirichlet(np.full(ok.sum(), 0.3))
        q = np.zeros(43)
        q[ok] = rng.dirichlet(np.full(ok.sum(), 0.5))
        visits = rng.multinomial(100, q)
        pi = (visits.astype(f32) / f32(100.0)).astype(f32)
        valid = sum(1 << m for m in range(43) if ok[m])
        out.append((pi, P.astype(f32), valid))
    return out


def _kl64(pi, P, valid):
    ok = S.bits(valid) & (pi > 0)
    p, q = pi.astype(np.float64)[ok], np.maximum(P, S.TINY).astype(np.float64)[ok]
    return max(float((p * (np.log(p) - np.log(q))).sum()), 0.0)


def test_record_kl_against_float64():
    worst, top = 0.0, 0.0
    for pi, P, valid in _pairs(3000, 2):
        kl = S.record_kl(pi, P, valid)
        assert kl.dtype == f32 and kl >= 0
        worst = max(worst, abs(float(kl) - _kl64(pi, P, valid)))
        top = max(top, float(kl))
    print("KL over 3000 (pi, P) pairs: max absolute error %.3g, largest KL %.3g" % (worst, top))
    assert worst <= 1e-5
    one_hot = np.zeros(43, f32); one_hot[7] = 1
    assert S.record_kl(one_hot, one_hot, 1 << 7) == 0.0


def test_the_weights_of_a_game_sum_to_its_record_count():
    rng = np.random.default_rng(3)
    worst = 0.0
    for n in (1, 2, 3, 17, 64, 65, 130, 700, 4096):
        for share in (0.25, 0.5, 1.0):
            kl = rng.gamma(0.7, 0.4, n).astype(f32)
            kl[rng.random(n) < 0.2] = 0
            if not kl.any():
                kl[0] = f32(0.1)
            w = S.game_weights(kl, share, 1e30)                # no cap binds
            assert w.dtype == f32 and (w >= f32(1.0) - f32(share)).all()
            d = abs(float(w.astype(np.float64).sum()) - n) / n
            worst = max(worst, d)
            assert d <= 1e-4, (n, share, d)
    print("|sum w - n| / n: max %.3g" % worst)
    assert (S.game_weights(np.zeros(5, f32), 0.5, 4.0) == 1).all()                       # S = 0: every record once
    assert (S.game_weights(np.array([0, 3, 0, 0], f32), 1.0, 2.5) == np.array([0, 2.5, 0, 0], f32)).all()   # the cap binds


def test_the_mean_copy_count_is_the_weight():
    n = 20000
    for w, seed in ((0.37, 5), (1.5, 6), (2.9375, 7), (0.03, 8)):
        w = f32(w)
        c = np.array([S.copies(w, seed, 1000 + i // 50, i % 50) for i in range(n)])
        fr = float(w) - int(w)
        se = np.sqrt(fr * (1 - fr) / n)
        print("w = %.4f: mean copies %.5f (%.2f standard errors off)" % (w, c.mean(), (c.mean() - float(w)) / se))
        assert set(c) <= {int(w), int(w) + 1}
        assert abs(c.mean() - float(w)) <= 6 * se
    for w in (0.0, 1.0, 2.0, 64.0):                            # an exact integer never gets an extra copy
        assert {S.copies(f32(w), 9, s, r) for s in range(40) for r in range(40)} == {int(w)}


def test_the_coin_is_not_the_playout_caps():
    """the same seed for both, the same game seeds, record ordinal = decision: the extra copy of w = 0.5 against full / fast at 0.5"""
    n = 20000
    for seed in (0, 99):
        a = np.array([S.copies(f32(0.5), seed, 7000 + i // 100, i % 100) for i in range(n)], float)
        b = np.array([R.coin(0.5, seed, 7000 + i // 100, i % 100) for i in range(n)], float)
        r = np.corrcoef(a, b)[0, 1]
        print("seed %d: correlation of the copy coin with the cap's coin %.4f (bound %.4f)" % (seed, r, 6 / np.sqrt(n)))
        assert abs(r) <= 6 / np.sqrt(n)
