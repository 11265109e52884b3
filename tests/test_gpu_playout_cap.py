"""GPU: playout cap randomisation in device self-play (azr_selfplay_set_playout_cap, azr_selfplay_decision_kind,
azr_debug_playout_cap).  The contract is include/azr.h's: a coin of (cap seed, game seed, decision) makes a decision full (the whole
budget, sampled root noise, one record) or fast (the small budget, the constant noise term, no record); everything else is the
uncapped loop.  Checked here: off is the engine without the call; the coin against its Python restatement (tests/playout_cap_ref.py);
the gating alone (equal budgets); mixed budgets against the oracle's pieces with the device net called back; games are a function of
their seeds alone; noise only where the search is full; a never-full engine plays the small-budget engine's games; argument checks."""
import ctypes as C

import numpy as np
import pytest

import azr_testlib as T
import playout_cap_ref as R
import selfplay_retrace as SR
from gpu_common import pkg

pytestmark = pytest.mark.gpu
BASE = 4242


def _selfplay(eng, games, quota=None, runs=400):
    """self-play of new games (a quota of them, or without an end) until `games` games are over; (records, counters)"""
    if quota:
        eng.selfplay_start_games(BASE, quota)
    else:
        eng.selfplay_start(BASE)
    r, c = SR.play_out(eng, games, 64, runs, exact=bool(quota))
    assert len(r) == c["samples"]
    return r, c


# ---- 1. off is today ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", [1, 2])
def test_off_is_the_engine_that_never_called_it(threads):
    P = pkg()
    G = 6
    flat = T.make_net_flat(1, seed=11, perturb_bn=True)
    out = []
    for cap in (None, (1.0, 2, 7), (0.5, 0, 7)):
        eng = P.Engine(G, blocks=1, sims=6, dtype=P.NET_F32, max_game_rounds=36, threads=threads)
        eng.set_weights(flat)
        if cap:
            eng.selfplay_set_playout_cap(*cap)
        r, c = _selfplay(eng, G)
        assert eng.decision_kind().all()
        out.append((r.tobytes(), c))
        eng.close()
    assert len(out[0][0]) > 0
    for blob, c in out[1:]:
        assert blob == out[0][0] and c == out[0][1]


# ---- 2. the coin -------------------------------------------------------------------------------------------------------------
def test_the_coin_is_the_headers_formula():
    P = pkg()
    eng = P.Engine(2, blocks=1, sims=6, dtype=P.NET_F32)
    seeds, decs = np.arange(256, dtype=np.uint32), np.arange(256, dtype=np.uint32)
    s, d = np.repeat(seeds, 256), np.tile(decs, 256)
    got = eng.debug_playout_cap(0.25, 99, s, d).reshape(256, 256)
    want = R.coin_grid(0.25, 99, seeds, decs)
    assert (got == want).all()
    share = got.mean()
    print("full share on the grid:", share)
    assert abs(share - 0.25) <= 5 * np.sqrt(0.25 * 0.75 / 65536)          # 5 binomial standard deviations: +- 0.0085
    assert not eng.debug_playout_cap(0.0, 99, s, d).any()
    assert eng.debug_playout_cap(1.0, 99, s, d).all()
    other = eng.debug_playout_cap(0.25, 100, s, d).reshape(256, 256)
    assert (other == R.coin_grid(0.25, 100, seeds, decs)).all() and (other != got).any()
    # odd lengths: the kernel's last block is partial
    for n in (1, 63, 65):
        assert (eng.debug_playout_cap(0.25, 99, s[:n], d[:n]) == want.reshape(-1)[:n]).all()
    eng.close()


# ---- 3. gating alone ---------------------------------------------------------------------------------------------------------
def _split_games(orc, recs, seeds):
    """the ring of a quota run with one game per seed, cut into games: a game's first record shows the deal of its seed"""
    start = {}
    for seed in seeds:
        r, s = T.OrcRng(), T.OrcState()
        orc.orc_rng_seed(C.byref(r), seed)
        orc.orc_new_game(C.byref(s), C.byref(r))
        x = np.zeros(88, np.uint8)
        orc.orc_encode(C.byref(s), T.ptr(x))
        hits = [i for i in range(len(recs)) if recs[i, 0] == s.cur and (recs[i, 1:89] == x).all()]
        assert len(hits) == 1, (seed, hits)
        start[seed] = hits[0]
    cuts = sorted(start.values()) + [len(recs)]
    assert cuts[0] == 0
    return {seed: recs[start[seed]:cuts[cuts.index(start[seed]) + 1]] for seed in seeds}


@pytest.mark.parametrize("threads", [1, 2])
def test_equal_budgets_only_gate_the_records(orc, threads):
    P = pkg()
    G = 6
    flat = T.make_net_flat(1, seed=11, perturb_bn=True)
    out = []
    for prob in (1.0, 0.5):
        eng = P.Engine(G, blocks=1, sims=6, dtype=P.NET_F32, max_game_rounds=36, threads=threads)
        eng.set_weights(flat)
        eng.selfplay_set_playout_cap(prob, 6, 99)
        out.append(_selfplay(eng, G, quota=G))      # exactly the games of seeds BASE .. BASE + 5, each played to its end
        eng.close()
    (all_recs, c1), (cap_recs, c2) = out
    assert c1["games_finished"] == c2["games_finished"] == G
    games = _split_games(orc, all_recs, range(BASE, BASE + G))
    blob, full_total = cap_recs.tobytes(), 0
    for seed, g in games.items():
        full = np.array([R.coin(0.5, 99, seed, d) for d in range(len(g))])
        assert 0 < full.sum() < len(g)
        assert g[full].tobytes() in blob, f"game {seed}: its full decisions are not a contiguous run of the capped engine's records"
        full_total += int(full.sum())
    assert c2["decisions"] == c1["decisions"] == sum(len(g) for g in games.values())
    assert c2["simulations"] == c1["simulations"]
    assert c2["samples"] == full_total == len(cap_recs)


# ---- 4. mixed budgets against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", [1, 2])
def test_mixed_budgets_vs_oracle(threads):
    mixed_budgets_vs_oracle(threads, 6, T.make_net_flat(1, seed=11, perturb_bn=True))


def test_sharp_mixed_budgets_vs_oracle():
    """the same on the sharp net of that seed (two games, two search threads): fast searches of 2 simulations on priors of exactly 0"""
    mixed_budgets_vs_oracle(2, 2, T.make_sharp_net_flat(1, seed=11))


def mixed_budgets_vs_oracle(threads, G, flat):
    P = pkg()
    sims, fast = 6, 2
    eng = P.Engine(G, blocks=1, sims=sims, dtype=P.NET_F32, max_game_rounds=36, threads=threads)
    eng.set_weights(flat)
    eng.selfplay_set_playout_cap(0.5, fast, 99)
    recs, c = _selfplay(eng, G, quota=G)             # exactly the games of seeds BASE .. BASE + 5, each played to its end
    assert c["games_finished"] == G
    blob = recs.tobytes()

    @T.EVAL_FN
    def hip_eval(ctx, in88, pi, v):
        x = np.ctypeslib.as_array(in88, shape=(88,)).copy()[None]
        p, vv = eng.predict(x)
        C.memmove(pi, p.ctypes.data, 43 * 4)
        v[0] = float(vv[0])

    cfg = T.default_settings(mcts_simulations=sims, max_game_rounds=36, mcts_threads=threads)
    tot = dict(decisions=0, simulations=0, samples=0)
    for g in range(G):
        want, kinds, st, nsims = R.selfplay_game(cfg, BASE + g, hip_eval, 0.5, fast, 99)
        full, nfast = int(kinds.sum()), int((kinds == 0).sum())
        assert full >= 10 and nfast >= 10, (g, full, nfast)          # the condition on the inputs: both kinds, many times
        assert nsims == (sims - sims % threads) * full + (fast - fast % threads) * nfast
        assert len(want) == full and want.tobytes() in blob, f"game {g}: record stream not found in the device's output"
        tot["decisions"] += len(kinds); tot["simulations"] += nsims; tot["samples"] += full
    # a quota run stops with its games, so the counters are those of exactly these six
    assert {k: c[k] for k in tot} == tot
    eng.close()


# ---- 5. a function of the seeds alone -----------------------------------------------------------------------------------------
def test_capped_quota_selfplay_is_a_function_of_the_seeds_alone():
    P = pkg()
    N, out = 60, []
    for G in (40, 7):
        eng = P.Engine(G, blocks=2, sims=8, dtype=P.NET_BF16, threads=2, max_game_rounds=40)
        eng.init_random(5)
        eng.selfplay_set_playout_cap(0.5, 2, 7)
        r, c = _selfplay(eng, N, quota=N, runs=4000)
        assert c["games_finished"] == N and 0 < c["samples"] < c["decisions"]
        out.append((r[np.lexsort(r.T[::-1])], c["decisions"], c["simulations"]))   # records sorted bytewise
        eng.close()
    assert out[0][0].shape == out[1][0].shape and len(out[0][0]) > 100
    assert (out[0][0] == out[1][0]).all() and out[0][1:] == out[1][1:]


# ---- 6. noise only where the search is full -----------------------------------------------------------------------------------
def test_root_noise_is_drawn_for_full_roots_only():
    P = pkg()
    G = 8
    eng = P.Engine(G, blocks=1, sims=6, dtype=P.NET_F32, threads=2, max_game_rounds=36)
    eng.init_random(5)
    dnv = np.float32(eng.settings.dir_noise_value)
    eng.selfplay_set_dirichlet(0.3, 5)
    eng.selfplay_set_playout_cap(0.5, 2, 7)
    eng.selfplay_start(BASE)
    seen = [0, 0]
    for step in range(41):
        if step:
            eng.selfplay_run(3)
        eta, kind, valid = eng.root_noise(), eng.decision_kind(), eng.valid_moves()
        for g in range(G):
            seen[int(kind[g])] += 1
            if kind[g]:
                ok = np.array([(int(valid[g]) >> m) & 1 for m in range(43)], bool)
                assert ok.any() and (eta[g][~ok] == 0).all(), (step, g)
                assert abs(float(eta[g].astype(np.float64).sum()) - 1.0) <= 2.0 ** -23, (step, g)
            else:
                assert (eta[g] == dnv).all(), (step, g)
    assert seen[0] > 0 and seen[1] > 0, seen
    c = eng.counters()
    assert c["errors"] == 0 and c["decisions"] > 0
    eng.close()


# ---- 7. noise off on fast decisions, end to end -------------------------------------------------------------------------------
def test_a_never_full_engine_plays_the_small_budgets_games():
    """full_prob = 0 with Dirichlet noise set: every decision is fast, so its root vector is the constant and its budget the fast
    one — the games of an engine created with that budget, without noise and without a cap; and no record is ever written.  Both
    engines get the same node pool, which is otherwise sized from mcts_simulations."""
    P = pkg()
    G = 6
    flat = T.make_net_flat(1, seed=11, perturb_bn=True)
    a = P.Engine(G, blocks=1, sims=6, dtype=P.NET_F32, threads=1, max_game_rounds=36, node_capacity=112)
    b = P.Engine(G, blocks=1, sims=2, dtype=P.NET_F32, threads=1, max_game_rounds=36, node_capacity=112)
    a.set_weights(flat); b.set_weights(flat)
    a.selfplay_set_dirichlet(0.3, 5)
    a.selfplay_set_playout_cap(0.0, 2, 7)
    a.selfplay_start(BASE); b.selfplay_start(BASE)
    for step in range(30):
        a.selfplay_run(8); b.selfplay_run(8)
        assert a.get_states().tobytes() == b.get_states().tobytes(), step
        assert (a.get_rng() == b.get_rng()).all(), step
        assert not a.decision_kind().any() and b.decision_kind().all()
        assert len(a.drain()) == 0
    ca, cb = a.counters(), b.counters()
    assert ca["decisions"] == cb["decisions"] > 0 and ca["simulations"] == cb["simulations"]
    assert ca["samples"] == 0 and ca["errors"] == cb["errors"] == 0 and ca["nodes_dropped"] == cb["nodes_dropped"] == 0
    a.close(); b.close()


# ---- 8. argument checks --------------------------------------------------------------------------------------------------------
def test_argument_checks_and_a_running_selfplay_never_sees_a_change():
    P = pkg()
    G = 4
    eng = P.Engine(G, blocks=1, sims=6, dtype=P.NET_F32, threads=2, max_game_rounds=36)
    eng.init_random(5)
    for bad in ((float("nan"), 2, 0), (-0.25, 2, 0), (0.5, 1, 0), (0.5, 7, 0)):     # NaN, negative, fast < T, fast > sims
        with pytest.raises(P.AzrError) as e:
            eng.selfplay_set_playout_cap(*bad)
        assert e.value.code == 1 and "azr_selfplay_set_playout_cap" in str(e.value), bad
    eng.selfplay_set_playout_cap(1.0, 1, 0)      # off: the fast budget is not looked at
    eng.selfplay_set_playout_cap(0.5, -3, 0)
    with pytest.raises(P.AzrError) as e:
        eng.debug_playout_cap(float("nan"), 0, np.zeros(1, np.uint32), np.zeros(1, np.uint32))
    assert e.value.code == 1
    assert eng.decision_kind().all()             # not in self-play
    # never full, started; switched off while it runs: the running self-play still writes nothing
    eng.selfplay_set_playout_cap(0.0, 2, 7)
    eng.selfplay_start(BASE)
    eng.selfplay_set_playout_cap(1.0, 0, 7)
    for _ in range(6):
        eng.selfplay_run(32)
    c = eng.counters()
    assert c["decisions"] > 20 and c["samples"] == 0 and len(eng.drain()) == 0 and not eng.decision_kind().any()
    # the next start reads the setting: every decision is full again
    eng.selfplay_start(BASE)
    assert eng.decision_kind().all()
    r, c = _selfplay(eng, 1, runs=400)
    assert c["samples"] > 0 and len(r) == c["samples"]
    eng.close()
