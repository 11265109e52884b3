"""GPU: policy surprise weighting of the self-play records (azr_selfplay_set_surprise_weighting, azr_debug_surprise_weights).  The
contract is include/azr.h's; tests/surprise_ref.py restates it in np.float32.  Checked here: the rule on the device against the
restatement, bit for bit; device self-play against the same games retraced decision by decision through the host-stepped entry points,
each record repeated by the restatement's copy count (plain at one and two search threads, and with a playout cap, Dirichlet noise,
forced playouts and pruning); weighting on against off; slot independence; off is the engine that never called it; argument checks.
Engines of 8 games, one block, NET_F32, 8 simulations, on the late golden positions of tests/selfplay_retrace.py."""
import numpy as np
import pytest

import selfplay_retrace as SR
import surprise_ref as S
from gpu_common import pi_of, pkg

pytestmark = pytest.mark.gpu
f32 = np.float32
BASE, NSEED, CSEED, SIMS, FAST, ALPHA, K, QUOTA = 9100, 77, 99, 8, 4, 0.3, 2.0, 4
SHARE, MAXW, PSEED = 0.75, 4.0, 31


# ---- 1. the rule, bit for bit ------------------------------------------------------------------------------------------------------
def _row(rng, ok):
    """(pi from 20 multinomial visits, Dirichlet(0.3) P) over the legal moves `ok`: pi has entries of 0 wherever a move got no visit"""
    P, q = np.zeros(43), np.zeros(43)
    P[ok] = rng.dirichlet(np.full(ok.sum(), 0.3))
    q[ok] = rng.dirichlet(np.full(ok.sum(), 0.5))
    return (rng.multinomial(20, q).astype(f32) / f32(20.0)).astype(f32), P.astype(f32)


def _rule_games():
    """[(name, pi [n, 43], prior [n, 43], valid [n])]"""
    rng = np.random.default_rng(17)
    games = []
    for n in (1, 2, 63, 64, 65, 130):
        pi, pr, va = [], [], []
        for r in range(n):
            ok = np.ones(43, bool) if r % 3 == 0 else rng.random(43) < 0.35
            if r % 7 == 1 or not ok.any():                          # one legal move
                ok = np.zeros(43, bool); ok[int(rng.integers(43))] = True
            a, b = _row(rng, ok)
            if r % 5 == 2:                                          # P of 0 and subnormal P under moves the search visited
                hit = np.nonzero(a > 0)[0]
                b[hit[0]] = 0
                if len(hit) > 1:
                    b[hit[1]] = f32(1e-40)
            pi.append(a); pr.append(b); va.append(sum(1 << m for m in range(43) if ok[m]))
        games.append(("random %d" % n, np.array(pi, f32), np.array(pr, f32), np.array(va, np.uint64)))
    hot = np.zeros((9, 43), f32); hot[np.arange(9), np.arange(9) * 4] = 1
    games.append(("one-hot", hot, hot.copy(), (np.uint64(1) << (np.arange(9, dtype=np.uint64) * np.uint64(4)))))
    # one surprised record among records the net knew: its weight is n * share, far above any cap
    pi = np.tile(hot[:1], (20, 1)); pr = pi.copy()
    pr[11] = 0; pr[11, 5] = 1
    games.append(("capped", pi, pr, np.full(20, (1 << 43) - 1, np.uint64)))
    # two equal records: KL_r / S = 1/2 exactly, w = (1 - share) + share
    a, b = _row(rng, np.ones(43, bool))
    games.append(("twins", np.array([a, a]), np.array([b, b]), np.full(2, (1 << 43) - 1, np.uint64)))
    return games


@pytest.mark.parametrize("share,max_weight,seed", [(0.5, 4.0, 0), (1.0, 4.0, 12345), (0.75, 64.0, 0xFFFFFFFF)])
def test_the_rule_on_the_device_is_the_restatement(share, max_weight, seed):
    games = _rule_games()
    seeds = np.array([5 + 1000003 * i for i in range(len(games))], np.uint32)
    P = pkg()
    eng = P.Engine(2, blocks=1, sims=SIMS, dtype=P.NET_F32)
    kl, w, c = eng.debug_surprise_weights(share, max_weight, seed, np.concatenate([g[1] for g in games]), np.concatenate([g[2] for g in games]),
                                          np.concatenate([g[3] for g in games]), [len(g[1]) for g in games], seeds)
    eng.close()
    at = 0
    for (name, pi, pr, va), gs in zip(games, seeds):
        n = len(pi)
        want_kl = np.array([S.record_kl(pi[r], pr[r], va[r]) for r in range(n)], f32)
        want_w, want_c = S.game_copies(want_kl, share, max_weight, seed, int(gs))
        got = kl[at:at + n], w[at:at + n], c[at:at + n]
        assert got[0].tobytes() == want_kl.tobytes(), (name, got[0], want_kl)
        assert got[1].tobytes() == want_w.tobytes(), (name, got[1], want_w)
        assert (got[2] == want_c).all(), (name, got[2], want_c)
        if name == "one-hot":
            assert not want_kl.any() and (got[1] == 1).all() and (got[2] == 1).all()
        if name == "capped" and max_weight == 4.0:                   # (1 - share) + share * 20 is above 4, and below 64
            assert got[1][11] == f32(max_weight) and got[2][11] == int(max_weight) and (np.delete(got[1], 11) == f32(1.0) - f32(share)).all()
        if name == "twins" and share == 0.5:
            assert (got[1] == 1).all() and (got[2] == 1).all()       # an exact integer: never an extra copy
        if name.startswith("random") and n >= 63:
            assert (got[2] == 0).any() and (got[2] >= 2).any(), name
        at += n
    assert at == len(kl)


# ---- 2. self-play equals the host-stepped composition, each record repeated by its copy count -----------------------------------------
def _run(threads, full, on):
    """the four late games; `full`: under a playout cap, Dirichlet noise, forced playouts and pruning; on = False: the setter is never
    called"""
    return SR.Run(BASE, QUOTA, threads, SIMS, surprise=(SHARE, MAXW, PSEED) if on else None,
                  **(dict(fast=FAST, cap=(0.5, CSEED), dirichlet=(ALPHA, NSEED), forced=(K, True)) if full else {}))


def _expected(threads, full):
    """per game (records, copies) by the restatement on the retrace's policies and priors, and the retrace's totals"""
    games, tot = SR.cached("retrace", _run(threads, full, True))
    out = []
    for g, game in enumerate(games):
        kl = np.array([S.record_kl(pi, pr, va) for pi, pr, va in zip(pi_of(game.records), game.prior, game.valid)], f32)
        out.append((game.records, S.game_copies(kl, SHARE, MAXW, PSEED, BASE + g)[1]))
    return out, tot


@pytest.mark.parametrize("threads,full", [(1, False), (2, False), (2, True)])
def test_selfplay_is_the_host_stepped_composition_repeated_by_the_copies(threads, full):
    recs, c = SR.cached("selfplay", _run(threads, full, True))
    games, tot = _expected(threads, full)
    allc = np.concatenate([cp for _, cp in games])
    print("records per game:", [len(r) for r, _ in games], "copies:", [cp.tolist() for _, cp in games], tot)
    # a condition of the test, not a measurement: the games hold a record that is left out and one that is written more than once
    assert (allc == 0).any() and (allc >= 2).any(), np.bincount(allc)
    SR.assert_streams(recs, c, games, tot)
    assert len(recs) == int(allc.sum())


# ---- 3. on against off ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads,full", [(2, False), (2, True)])
def test_weighting_only_repeats_and_leaves_out_records(threads, full):
    on, c1 = SR.cached("selfplay", _run(threads, full, True))
    off, c0 = SR.cached("selfplay", _run(threads, full, False))
    for key in ("games_finished", "decisions", "simulations", "evaluations", "levels"):
        assert c0[key] == c1[key], key
    assert c0["samples"] == len(off) and c1["samples"] == len(on)
    rows_on = {r.tobytes() for r in on}
    rows_off = [r.tobytes() for r in off]
    assert rows_on <= set(rows_off)
    games, _ = _expected(threads, full)
    want = {}
    for recs, cp in games:
        for r, n in zip(recs, cp):
            want[r.tobytes()] = want.get(r.tobytes(), 0) + int(n)
    assert set(want) == set(rows_off)
    missing = [b for b in set(rows_off) if b not in rows_on]
    assert missing and all(want[b] == 0 for b in missing)
    count = {}
    for r in on:
        count[r.tobytes()] = count.get(r.tobytes(), 0) + 1
    assert count == {b: n for b, n in want.items() if n}


# ---- 4. slot independence ---------------------------------------------------------------------------------------------------------
def test_a_quota_writes_the_same_records_on_two_and_on_eight_slots():
    _, decisions, _, samples = SR.quota_on_slots((2, 8), lambda eng: eng.selfplay_set_surprise_weighting(SHARE, MAXW, PSEED), SIMS, BASE)
    print("records %d of %d decisions" % (samples, decisions))
    assert samples != decisions


# ---- 5. off is the engine that never called it ------------------------------------------------------------------------------------
def test_off_is_the_engine_that_never_called_it():
    def meddle(i, eng):
        if i == 0:                                                # on again while it runs
            assert eng.counters()["games_finished"] < QUOTA
            eng.selfplay_set_surprise_weighting(SHARE, MAXW, PSEED)

    def on_then_off(eng):                                         # a non-zero setting first, then off before the start
        eng.selfplay_set_surprise_weighting(SHARE, MAXW, PSEED)
        eng.selfplay_set_surprise_weighting(0.0, MAXW, PSEED)

    run = _run(2, False, False)
    never, c0 = SR.cached("selfplay", run)
    eng = SR.selfplay(run, on_then_off)
    recs, c = SR.play_out(eng, QUOTA, 16, 400, after_run=meddle)
    assert recs.tobytes() == never.tobytes() and c == c0
    # the next start reads the setting
    SR.place(eng, run)
    again, c = SR.play_out(eng, QUOTA, 16, 400)
    eng.close()
    on, c1 = SR.cached("selfplay", _run(2, False, True))
    assert on.tobytes() != never.tobytes()
    assert again.tobytes() == on.tobytes() and c == c1


# ---- 6. argument errors -----------------------------------------------------------------------------------------------------------
def test_argument_errors():
    P = pkg()
    eng = P.Engine(2, blocks=1, sims=4, dtype=P.NET_F32, threads=2)
    L = eng.L
    assert L.azr_selfplay_set_surprise_weighting(None, 0.5, 4.0, 0) == 3        # AZR_E_BAD_HANDLE
    assert L.azr_debug_surprise_weights(None, 0.5, 4.0, 0, None, None, None, None, None, 0, None, None, None) == 3
    nan = float("nan")
    for bad in ((nan, 4.0), (1.5, 4.0), (0.5, nan), (0.5, 0.5), (0.5, 64.5), (1.0, -1.0)):
        with pytest.raises(P.AzrError) as e:
            eng.selfplay_set_surprise_weighting(*bad)
        assert e.value.code == 1 and "azr_selfplay_set_surprise_weighting" in str(e.value), bad
    eng.selfplay_set_surprise_weighting(0.0, 0.0)                 # off: the cap is not looked at
    eng.selfplay_set_surprise_weighting(-2.0, 1000.0)
    eng.selfplay_set_surprise_weighting(1.0, 1.0); eng.selfplay_set_surprise_weighting(0.5, 64.0); eng.selfplay_set_surprise_weighting(0.0)
    row, ok = np.full((1, 43), 1 / 43, f32), np.array([(1 << 43) - 1], np.uint64)
    for bad in ((0.0, 4.0), (nan, 4.0), (1.5, 4.0), (0.5, 0.5), (0.5, 65.0)):
        with pytest.raises(P.AzrError) as e:
            eng.debug_surprise_weights(bad[0], bad[1], 0, row, row, ok, [1], [0])
        assert e.value.code == 1 and "azr_debug_surprise_weights" in str(e.value), bad
    assert L.azr_debug_surprise_weights(eng.h, 0.5, 4.0, 0, None, None, None, None, None, 1, None, None, None) == 1
    kl, w, c = eng.debug_surprise_weights(0.5, 4.0, 0, row, row, ok, [1], [0])
    assert kl[0] == 0 and w[0] == 1 and c[0] == 1
    eng.close()
