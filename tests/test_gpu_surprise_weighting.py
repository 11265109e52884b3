"""GPU: policy surprise weighting of the self-play records (azr_selfplay_set_surprise_weighting, azr_debug_surprise_weights).  The
contract is include/azr.h's; tests/surprise_ref.py restates it in np.float32.  Checked here: the rule on the device against the
restatement, bit for bit; device self-play against the same games retraced decision by decision through the host-stepped entry points,
each record repeated by the restatement's copy count (plain at one and two search threads, and with a playout cap, Dirichlet noise,
forced playouts and pruning); weighting on against off; slot independence; off is the engine that never called it; argument checks.
Engines of 8 games, one block, NET_F32, 8 simulations, on the late golden positions of the forced-playouts test."""
import numpy as np
import pytest

import azr_testlib as T
import playout_cap_ref as R
import surprise_ref as S
from gpu_common import pkg
from test_gpu_forced_playouts import _late_positions

pytestmark = pytest.mark.gpu
f32 = np.float32
G = 8
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
def _engine(threads, slots=G):
    P = pkg()
    eng = P.Engine(slots, blocks=1, sims=SIMS, dtype=P.NET_F32, threads=threads)
    eng.set_weights(T.make_net_flat(1, seed=11, perturb_bn=True))
    return eng


def _selfplay(threads, full, share, meddle=False):
    """the four late games in device self-play; `full`: under a playout cap, Dirichlet noise, forced playouts and pruning; share = None:
    the setter is never called.  meddle: weighting is switched on while the self-play runs (which must change nothing)"""
    eng = _engine(threads)
    states, rngs = _late_positions()
    eng.set_states(states)
    eng.set_rng(rngs)
    if full:
        eng.selfplay_set_dirichlet(ALPHA, NSEED)
        eng.selfplay_set_forced_playouts(K, True)
        eng.selfplay_set_playout_cap(0.5, FAST, CSEED)
    if share is not None:
        if meddle:
            eng.selfplay_set_surprise_weighting(SHARE, MAXW, PSEED)   # a non-zero setting first, then off
        eng.selfplay_set_surprise_weighting(share, MAXW, PSEED)
    eng.selfplay_start_games_from_states(BASE, QUOTA)
    recs = []
    for i in range(400):
        eng.selfplay_run(16)
        if meddle and i == 0:
            assert eng.counters()["games_finished"] < QUOTA
            eng.selfplay_set_surprise_weighting(SHARE, MAXW, PSEED)
        recs.append(eng.drain())
        c = eng.counters()
        if c["games_finished"] + c["errors"] >= QUOTA:
            break
    c = eng.counters()
    assert c["games_finished"] == QUOTA and c["errors"] == 0 and c["nodes_dropped"] == 0 and c["records_dropped"] == 0, c
    return np.concatenate(recs), c, eng


def _retrace(threads, full):
    """the same four games through azr_mcts_*, as the forced-playouts test retraces them, keeping each recorded decision's prior row
    and legal moves: per game (records [n, 265], KL [n])"""
    eng = _engine(threads)
    states, rngs = _late_positions()
    dnv, thr = f32(eng.settings.dir_noise_value), eng.settings.temperature_threshold
    games, tot = [], dict(decisions=0, simulations=0)
    for g in range(QUOTA):
        eng.set_states(np.repeat(states[g:g + 1], G, 0))          # every slot retraces game g; slot 0 is read
        eng.set_rng(np.full(G, rngs[g], np.uint32))
        eng.mcts_clear()
        recs, kls, d = [], [], 0
        while True:
            whole = R.coin(0.5, CSEED, BASE + g, d) if full else True
            valid = eng.valid_moves()
            if full:
                eta = eng.debug_root_noise(ALPHA, NSEED, [BASE + g], [d], valid[:1]) if whole else np.full((1, 43), dnv, f32)
                eng.set_root_noise(np.repeat(eta, G, 0))
                eng.set_forced_playouts(K if whole else 0.0)
                eng.set_simulations(SIMS if whole else FAST)
            eng.simulate()
            st = eng.get_states()[0]
            prior = eng.root_stats()[2][0]
            pi = eng.pruned_policy()[0][0] if full else eng.policy()[0]
            mv = eng.pick(sample=not (int(st[144]) + 256 * int(st[145]) > thr))
            if whole:
                rec = np.zeros(265, np.uint8)
                rec[0] = st[146]
                rec[1:89] = eng.encode()[0]
                rec[93:265] = pi.view(np.uint8)
                recs.append(rec)
                kls.append(S.record_kl(pi, prior, valid[0]))
            assert (eng.make_moves(mv) == 0).all()
            budget = SIMS if whole else FAST
            d += 1; tot["decisions"] += 1; tot["simulations"] += budget - budget % threads
            status = int(eng.status()[0])
            if status != -1:
                break
            assert d < 2000
        for rec in recs:
            z = 0.0 if status == -2 else (1.0 if int(rec[0]) == status else -1.0)
            rec[89:93] = np.array([z], f32).view(np.uint8)
        games.append((np.array(recs, np.uint8).reshape(len(recs), 265), np.array(kls, f32)))
    eng.close()
    return games, tot


_cache = {}


def _cached(kind, threads, full):
    key = (kind, threads, full)
    if key not in _cache:
        if kind == "retrace":
            _cache[key] = _retrace(threads, full)
        else:
            recs, c, eng = _selfplay(threads, full, SHARE if kind == "on" else None)
            eng.close()
            _cache[key] = (recs, c)
    return _cache[key]


def _expected(threads, full):
    """per game (records, copies) by the restatement, and the retrace's totals"""
    games, tot = _cached("retrace", threads, full)
    return [(recs, S.game_copies(kl, SHARE, MAXW, PSEED, BASE + g)[1]) for g, (recs, kl) in enumerate(games)], tot


@pytest.mark.parametrize("threads,full", [(1, False), (2, False), (2, True)])
def test_selfplay_is_the_host_stepped_composition_repeated_by_the_copies(threads, full):
    recs, c = _cached("on", threads, full)
    games, tot = _expected(threads, full)
    allc = np.concatenate([cp for _, cp in games])
    print("records per game:", [len(r) for r, _ in games], "copies:", [cp.tolist() for _, cp in games], tot)
    # a condition of the test, not a measurement: the games hold a record that is left out and one that is written more than once
    assert (allc == 0).any() and (allc >= 2).any(), np.bincount(allc)
    blob = recs.tobytes()
    for g, (want, cp) in enumerate(games):
        stream = np.repeat(want, cp, axis=0)
        assert len(want) > 0 and (len(stream) == 0 or stream.tobytes() in blob), f"game {g}: its weighted record stream is not in the device's output"
    assert len(recs) == int(allc.sum()) == c["samples"]
    assert {k: c[k] for k in tot} == tot


# ---- 3. on against off ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads,full", [(2, False), (2, True)])
def test_weighting_only_repeats_and_leaves_out_records(threads, full):
    on, c1 = _cached("on", threads, full)
    off, c0 = _cached("off", threads, full)
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
    P = pkg()
    N, out = 6, []
    for slots in (2, 8):
        eng = P.Engine(slots, blocks=1, sims=SIMS, dtype=P.NET_F32, threads=2, max_game_rounds=36)
        eng.set_weights(T.make_net_flat(1, seed=11, perturb_bn=True))
        eng.selfplay_set_surprise_weighting(SHARE, MAXW, PSEED)
        eng.selfplay_start_games(BASE, N)
        recs = []
        for _ in range(4000):
            eng.selfplay_run(64)
            recs.append(eng.drain())
            c = eng.counters()
            if c["games_finished"] + c["errors"] >= N:
                break
        assert c["games_finished"] == N and c["errors"] == 0 and c["records_dropped"] == 0, c
        r = np.concatenate(recs)
        assert len(r) == c["samples"]
        out.append((r[np.lexsort(r.T[::-1])], c["decisions"], c["simulations"], c["samples"]))
        eng.close()
    print("records %d of %d decisions" % (out[0][3], out[0][1]))
    assert out[0][0].shape == out[1][0].shape and len(out[0][0]) > 50 and out[0][3] != out[0][1]
    assert (out[0][0] == out[1][0]).all() and out[0][1:] == out[1][1:]


# ---- 5. off is the engine that never called it ------------------------------------------------------------------------------------
def test_off_is_the_engine_that_never_called_it():
    never, c0 = _cached("off", 2, False)
    recs, c, eng = _selfplay(2, False, 0.0, meddle=True)          # on, then off before the start; on again while it runs
    assert recs.tobytes() == never.tobytes() and c == c0
    # the next start reads the setting
    states, rngs = _late_positions()
    eng.set_states(states)
    eng.set_rng(rngs)
    eng.selfplay_start_games_from_states(BASE, QUOTA)
    again = []
    for _ in range(400):
        eng.selfplay_run(16)
        again.append(eng.drain())
        c = eng.counters()
        if c["games_finished"] + c["errors"] >= QUOTA:
            break
    eng.close()
    on, c1 = _cached("on", 2, False)
    assert on.tobytes() != never.tobytes()
    assert np.concatenate(again).tobytes() == on.tobytes() and c == c1


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
