"""GPU: the Gumbel root search with sequential halving (azr_selfplay_set_gumbel, azr_mcts_set_gumbel, azr_mcts_set_root_gumbel,
azr_mcts_gumbel_policy / _pick, azr_debug_*).  The contract is include/azr.h's; tests/gumbel_ref.py restates it in np.float32.  Checked
here: the debug kernels against the restatement, bit for bit; a host-stepped search pass by pass against the restatement's selection,
the {6, 6, 2, 2} of the hand example, and the decision's pi and move over tree reuse; off is the engine that never called it; device
self-play against the same games retraced decision by decision through the host-stepped entry points (m = 4 and 16, one and two search
threads, and under surprise weighting and the value mix); slot independence; refusals.
Engines of 8 games, one block, NET_F32, budgets of 16 and 32."""
import numpy as np
import pytest

import azr_testlib as T
import gumbel_ref as G
import selfplay_retrace as SR
import surprise_ref as S
import value_mix_ref as V
from gpu_common import host_net, pi_of, pkg

pytestmark = pytest.mark.gpu
f32 = np.float32
SLOTS = 8
CV, CS, GSEED, BASE, QUOTA = 50.0, 0.5, 4242, 9300, 4
SHARE, MAXW, PSEED, QSHARE = 0.75, 4.0, 31, 0.5
ALL = (1 << 43) - 1


# ---- 1. the debug kernels, bit for bit ---------------------------------------------------------------------------------------------
def _engine(threads=1, sims=16, sharp=False):
    P = pkg()
    eng = P.Engine(SLOTS, blocks=1, sims=sims, dtype=P.NET_F32, threads=threads)
    eng.set_weights(host_net(sharp))
    return eng


def test_exp32_on_the_device_is_the_restatement():
    rng = np.random.default_rng(3)
    edge = np.array([0.0, -0.0, -104.0, -104.00001, -103.0, -87.5, -87.33655, -150.0, -1e30, -np.inf, -0.34657359, -0.3465736, -1e-8], f32)
    x = np.concatenate([edge, -rng.uniform(0, 104, 4096).astype(f32)])
    eng = _engine()
    got = eng.debug_exp32(x)
    eng.close()
    assert got.tobytes() == G.exp32(x).tobytes(), np.nonzero(got != G.exp32(x))


def test_the_draw_on_the_device_is_the_restatement():
    rng = np.random.default_rng(4)
    seeds = rng.integers(0, 1 << 32, 64, dtype=np.uint64).astype(np.uint32)
    dec = rng.integers(0, 300, 64).astype(np.uint32)
    valid = np.array([int(rng.integers(1, 1 << 43)) for _ in range(64)], np.uint64)
    greedy = np.zeros(64, np.uint8)
    greedy[[5, 17, 40]] = 1
    valid[[7, 8, 17]] = [1 << 0, 1 << 42, 1 << 20]                                   # one legal move (row 17: and greedy)
    valid[9] = ALL
    eng = _engine()
    got = eng.debug_root_gumbel(GSEED, seeds, dec, valid, greedy)
    eng.close()
    want = np.array([G.draw(GSEED, int(s), int(d), int(v), bool(gr)) for s, d, v, gr in zip(seeds, dec, valid, greedy)])
    assert got.tobytes() == want.tobytes()
    assert not got[[5, 17, 40]].any() and (got[7] != 0).sum() == 1 and (got[9] != 0).all()


def _select_rows(m, n):
    """synthetic rows for (m, n): random ones, then the rows that reach both fallbacks, a tie, and N0 != 0"""
    rng = np.random.default_rng(100 * m + n)
    rows = []

    def add(N, N0, act, Q, P, g, vhat, valid, i):
        rows.append((np.asarray(N, np.uint32), np.asarray(N0, np.uint32), np.asarray(act, np.uint32), np.asarray(Q, f32), np.asarray(P, f32),
                     np.asarray(g, f32), f32(vhat), int(valid), int(i)))

    for r in range(120):
        valid = int(rng.integers(1, 1 << 43)) if r % 3 else ALL
        N0 = rng.integers(0, 6, 43) * (r % 2)
        N = N0 + rng.integers(0, 1 + n // 4, 43) * (rng.random(43) < 0.5)
        act = (rng.random(43) < 0.1).astype(np.uint32)
        P = rng.dirichlet(np.full(43, 0.3)).astype(f32)
        if r % 5 == 0:
            P[rng.integers(0, 43, 5)] = 0.0                                         # a zero prior: the logit is ln32 of the smallest float
        g = np.array([G.draw(r, 7, 3, ALL)]).reshape(43)
        add(N, N0, act, rng.uniform(-1, 1, 43), P, g, rng.uniform(-1, 1), valid, rng.integers(0, n))
    z, P, g = np.zeros(43), np.full(43, 0.1, f32), np.zeros(43, f32)
    g[3], g[4] = 1.0, 1.0
    special = len(rows)
    add(z, z, z, z, P, g, 0.0, ALL, 0)                                              # a tie: the lowest index
    N = np.full(43, 7); N0 = N.copy(); N0[9] = 6
    add(N, N0, z, z, P, g, 0.0, ALL, min(m, 43), )                                  # N0 != 0: only move 9 has a search-local visit
    N = np.zeros(43); N[20] = 1
    add(N, z, z, z, P, g, 0.0, ALL, n - 1)                                          # nobody at cv: the largest count below it
    add(np.full(43, 60), z, z, z, P, g, 0.0, ALL, 0)                                # everybody above cv: all legal moves
    act = np.zeros(43); act[3] = 1
    add(z, z, act, z, P, g, 0.0, ALL, 1)                                            # a visit in flight counts
    cols = [np.array([r[k] for r in rows]) for k in range(9)]
    return cols, special


@pytest.mark.parametrize("m,n", [(4, 16), (16, 32), (43, 16), (1, 16)])
def test_the_selection_on_the_device_is_the_restatement(m, n):
    (N, N0, act, Q, P, g, vhat, valid, claim), special = _select_rows(m, n)
    want = [G.select(N[r], N0[r], act[r], Q[r], P[r], g[r], vhat[r], int(valid[r]), int(claim[r]), m, n, CV, CS) for r in range(len(valid))]
    if m == 4:   # conditions of the special rows, on the restatement
        assert want[special] == (3, 0) and want[special + 1][0] == 9 and want[special + 2][0] == 20 and want[special + 3] == (3, 0)
        assert want[special + 4] == (4, 0)
    eng = _engine()
    mv, cv = eng.debug_gumbel_select(m, n, CV, CS, N, N0, act, Q, P, g, vhat.astype(f32), valid.astype(np.uint64), claim)
    eng.close()
    assert mv.tolist() == [w[0] for w in want] and cv.tolist() == [w[1] for w in want]
    assert len(set(mv.tolist())) > 5 or m == 1


# ---- 2. host-stepped, pass by pass ---------------------------------------------------------------------------------------------------
def _stepped_search(eng, g, m, n):
    """one search under the vectors g through begin / leaves / azr_nn_predict / apply.  A launch's root-level selections are backed up by
    the next launch: the root visits every pass adds are checked against the restatement's selections on the previous pass's rows, game
    by game (a new root spends its first pass on its own expansion, one that tree reuse brought along does not).
    (N0, vhat, the final root_stats)"""
    Tn = eng.T
    eng.set_root_gumbel(g)
    vhat = eng.predict(eng.encode())[1]                                            # the net's value of every root, wherever it was expanded
    valid = eng.valid_moves()
    eng.mcts_begin()
    N0 = eng.root_stats()[0].copy()                                                # zeros for a root that is not in the tree
    claims = np.zeros(eng.G, np.int64)
    x, need, act = eng.mcts_leaves()
    prev, roots = eng.root_stats(), eng.get_states()
    in_tree = eng.node_stats(roots)[5]                                             # (a sharp net's prior row may be all zero: P.any() does not tell)
    while act:
        eng.mcts_apply(*eng.predict(x))
        x, need, act = eng.mcts_leaves()
        cur = eng.root_stats()
        for gi in range(eng.G):
            inflight, want = np.zeros(43, np.uint32), np.zeros(43, np.int64)
            if in_tree[gi] and claims[gi] < n:                                      # the root was in the tree: the launch before selected
                for th in range(Tn):
                    mv, _ = G.select(prev[0][gi], N0[gi], inflight, prev[1][gi], prev[2][gi], g[gi], vhat[gi], int(valid[gi]),
                                     int(claims[gi]) + th, m, n, CV, CS)
                    inflight[mv] += 1; want[mv] += 1
                claims[gi] += Tn
            assert ((cur[0][gi].astype(np.int64) - prev[0][gi]) == want).all(), (gi, claims[gi], cur[0][gi].astype(np.int64) - prev[0][gi], want)
        prev, in_tree = cur, eng.node_stats(roots)[5]
    assert (claims == n).all(), claims
    return N0, vhat, prev


@pytest.mark.parametrize("threads,m,n", [(1, 4, 16), (2, 4, 16), (2, 16, 32)])
def test_a_host_stepped_search_follows_the_restatement_pass_by_pass(threads, m, n):
    host_stepped_search_follows_the_restatement(threads, m, n, False)


def test_sharp_host_stepped_search_follows_the_restatement_pass_by_pass():
    """the smallest shape on the sharp net of that seed: logits of zero priors at the FLT_MIN clamp, completed Q from values of +-1"""
    host_stepped_search_follows_the_restatement(1, 4, 16, True)


def host_stepped_search_follows_the_restatement(threads, m, n, sharp):
    eng = _engine(threads, n, sharp)
    seeds = np.arange(4100, 4100 + SLOTS, dtype=np.uint32)
    eng.new_games(seeds)                                                           # setup phase: no descent ends in a finished game
    eng.set_gumbel(m, CV, CS)
    reused = 0
    for d in range(3):
        valid = eng.valid_moves()
        g = np.array([G.draw(GSEED, int(s), d, int(v)) for s, v in zip(seeds, valid)])
        assert eng.debug_root_gumbel(GSEED, seeds, np.full(SLOTS, d), valid, np.zeros(SLOTS)).tobytes() == g.tobytes()
        N0, vhat, (N, Q, P) = _stepped_search(eng, g, m, n)
        assert eng.root_gumbel().tobytes() == g.tobytes()
        ns = N.astype(np.int64) - N0
        assert (ns.sum(1) == n).all() and ((ns > 0).sum(1) <= m).all()
        if d == 0 and (threads, m, n) == (1, 4, 16) and not sharp:
            assert not N0.any() and all(sorted(r[r > 0].tolist()) == [2, 2, 6, 6] for r in ns), ns
        reused += int(N0.any(1).sum())
        pi, qhat = eng.gumbel_policy()
        mv = eng.gumbel_pick()
        for gi in range(SLOTS):
            wpi, wq = G.policy(N[gi], Q[gi], P[gi], vhat[gi], int(valid[gi]), CV, CS)
            assert pi[gi].tobytes() == wpi.tobytes() and qhat[gi].tobytes() == wq.tobytes(), (d, gi, pi[gi], wpi)
            assert mv[gi] == G.move(N[gi], N0[gi], Q[gi], P[gi], g[gi], vhat[gi], int(valid[gi]), CV, CS), (d, gi)
            assert ns[gi][mv[gi]] == ns[gi].max()
        assert (eng.make_moves(mv) == 0).all()
    print("roots that tree reuse brought along (N0 != 0):", reused)
    assert reused > 0
    eng.close()


# ---- 3. off is the parent ------------------------------------------------------------------------------------------------------------
def test_off_is_the_engine_that_never_called_it():
    def two_decisions(touch):
        eng = _engine(2, 16)
        eng.new_games(np.arange(4100, 4100 + SLOTS, dtype=np.uint32))
        touch(eng)
        out = []
        for _ in range(2):
            eng.simulate()
            mv = eng.pick(sample=True)
            out += [a.tobytes() for a in eng.root_stats()] + [eng.policy().tobytes(), mv.tobytes(), eng.get_rng().tobytes()]
            assert (eng.make_moves(mv) == 0).all()
        eng.close()
        return out

    def off(eng):
        eng.set_gumbel(0, CV, CS)
        eng.selfplay_set_gumbel(0, CV, CS, GSEED)

    assert two_decisions(lambda eng: None) == two_decisions(off)
    never = SR.quota_on_slots((8,), lambda eng: None, 16, BASE)
    called = SR.quota_on_slots((8,), off, 16, BASE)
    assert never[0].tobytes() == called[0].tobytes() and never[1:] == called[1:]


# ---- 4. device self-play is the host-stepped retrace -----------------------------------------------------------------------------------
_cache = {}


def _retrace(run, m):
    """SR.retrace's loop for a Gumbel self-play: per decision debug_root_gumbel -> set_root_gumbel -> simulate -> gumbel_policy into the
    record -> gumbel_pick as the move.  ([SR.Game], totals, the games' RNG streams after their last move)"""
    key = ("retrace", run._replace(surprise=None, value_mix=None), m)
    if key in _cache:
        return _cache[key]
    eng = SR.engine(run.threads, run.sims)
    eng.set_gumbel(m, CV, CS)
    states, rngs = SR.late_positions()
    thr = eng.settings.temperature_threshold
    games, streams, tot = [], [], dict(decisions=0, simulations=0, samples=0)
    for g in range(run.quota):
        eng.set_states(np.repeat(states[g:g + 1], SLOTS, 0))
        eng.set_rng(np.full(SLOTS, rngs[g], np.uint32))
        eng.mcts_clear()
        rows, d = [], 0
        while True:
            valid = eng.valid_moves()
            st = eng.get_states()[0]
            greedy = int(st[144]) + 256 * int(st[145]) > thr
            gum = eng.debug_root_gumbel(GSEED, [run.base + g], [d], valid[:1], [greedy])
            eng.set_root_gumbel(np.repeat(gum, SLOTS, 0))
            eng.simulate()
            n, q, prior = (a[0] for a in eng.root_stats())
            pi = eng.gumbel_policy()[0][0]
            mv = eng.gumbel_pick()
            rec = np.zeros(265, np.uint8)
            rec[0] = st[146]
            rec[1:89] = eng.encode()[0]
            rec[93:265] = pi.view(np.uint8)
            rows.append((rec, valid[0], n, q, prior))
            assert (eng.make_moves(mv) == 0).all()
            d += 1; tot["decisions"] += 1; tot["simulations"] += run.sims - run.sims % run.threads; tot["samples"] += 1
            status = int(eng.status()[0])
            if status != -1:
                break
            assert d < 2000
        streams.append(int(eng.get_rng()[0]))
        z = np.array([SR.outcome_z(status, int(row[0][0])) for row in rows], f32)
        for row, zr in zip(rows, z):
            row[0][89:93] = np.array([zr], f32).view(np.uint8)
        cols = [np.array([row[i] for row in rows], t).reshape(shape) for i, (t, shape) in
                enumerate(((np.uint8, (-1, 265)), (np.uint64, -1), (np.uint32, (-1, 43)), (f32, (-1, 43)), (f32, (-1, 43))))]
        games.append(SR.Game(cols[0], z, *cols[1:]))
    eng.close()
    _cache[key] = (games, tot, streams)
    return _cache[key]


def _selfplay(run, m):
    """(records, counters, the slots' RNG streams when the quota is over)"""
    key = ("selfplay", run, m)
    if key not in _cache:
        eng = SR.selfplay(run, lambda e: e.selfplay_set_gumbel(m, CV, CS, GSEED))
        recs, c = SR.play_out(eng, run.quota, 16, 400)
        _cache[key] = (recs, c, eng.get_rng()[:run.quota].tolist())
        eng.close()
    return _cache[key]


@pytest.mark.parametrize("m,threads,sims,psw,mix", [(4, 1, 16, False, False), (4, 2, 16, False, False), (16, 1, 16, False, False),
                                                    (16, 2, 32, False, False), (4, 2, 16, True, False), (4, 2, 16, False, True)])
def test_selfplay_is_the_host_stepped_retrace(m, threads, sims, psw, mix):
    run = SR.Run(BASE, QUOTA, threads, sims, surprise=(SHARE, MAXW, PSEED) if psw else None, value_mix=QSHARE if mix else None)
    recs, c, rng_dev = _selfplay(run, m)
    games, tot, rng_ref = _retrace(run, m)
    print("records per game:", [len(g.records) for g in games], tot)
    streams = []
    for g, game in enumerate(games):
        want, copies = game.records, None
        if psw:
            kl = np.array([S.record_kl(pi, pr, va) for pi, pr, va in zip(pi_of(game.records), game.prior, game.valid)], f32)
            copies = S.game_copies(kl, SHARE, MAXW, PSEED, BASE + g)[1]
        if mix:
            want = want.copy()
            for r in range(len(want)):
                q, has = V.root_value(game.N[r], game.Q[r], game.valid[r])
                want[r, 89:93] = np.array([V.blend(game.z[r], q, has, QSHARE)], f32).view(np.uint8)
        streams.append((want, copies))
    if psw:
        tot = dict(tot, samples=sum(int(np.sum(cp)) for _, cp in streams))
    SR.assert_streams(recs, c, streams, tot)
    # no rFloat: each game's dice stream after its last move is the retrace's
    assert rng_dev == rng_ref, (rng_dev, rng_ref)
    pi = pi_of(recs)
    assert np.abs(pi.astype(np.float64).sum(1) - 1).max() <= 43 * 2.0 ** -24


# ---- 5. slot independence --------------------------------------------------------------------------------------------------------------
def _quota(slots):
    """SR.quota_on_slots' quota under the Gumbel search on `slots` slots (one run per slot count and process)"""
    if ("quota", slots) not in _cache:
        _cache["quota", slots] = SR.quota_on_slots((slots,), lambda eng: eng.selfplay_set_gumbel(4, CV, CS, GSEED), 16, BASE, games=4)
    return _cache["quota", slots]


@pytest.mark.parametrize("slots", [2, 4])
def test_a_quota_writes_the_same_records_as_on_eight_slots(slots):
    recs, dec, sims, samples = _quota(8)
    other = _quota(slots)
    assert samples == dec and other[0].tobytes() == recs.tobytes() and other[1:] == (dec, sims, samples)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def test_argument_and_combination_refusals():
    P = pkg()
    eng = _engine(2, 16)
    L = eng.L
    assert L.azr_selfplay_set_gumbel(None, 4, CV, CS, 0) == 3 and L.azr_mcts_set_gumbel(None, 4, CV, CS) == 3       # AZR_E_BAD_HANDLE
    assert L.azr_mcts_set_root_gumbel(None, None) == 3 and L.azr_mcts_gumbel_pick(None, None) == 3
    nan, inf = float("nan"), float("inf")
    for setter, name in ((lambda *a: eng.selfplay_set_gumbel(*a, 7), "azr_selfplay_set_gumbel"), (eng.set_gumbel, "azr_mcts_set_gumbel")):
        for bad in ((44, CV, CS), (-1, CV, CS), (4, -1.0, CS), (4, CV, 0.0), (4, CV, -1.0), (4, nan, CS), (4, CV, inf), (0, nan, CS)):
            with pytest.raises(P.AzrError) as e:
                setter(*bad)
            assert e.value.code == 1 and name in str(e.value), bad
        setter(43, 0.0, 1e-3); setter(0, CV, CS)
    for call in (eng.gumbel_policy, eng.gumbel_pick):                              # no Gumbel search in force: AZR_E_STATE
        with pytest.raises(P.AzrError) as e:
            call()
        assert e.value.code == 7
    assert not eng.root_gumbel().any()
    # host-stepped: whichever setter comes second is refused
    eng.set_gumbel(4, CV, CS)
    for second in (lambda: eng.set_root_noise(np.full((SLOTS, 43), 0.3, f32)), lambda: eng.set_forced_playouts(2.0)):
        with pytest.raises(P.AzrError) as e:
            second()
        assert e.value.code == 1 and "Gumbel" in str(e.value)
    eng.set_root_noise(None); eng.set_forced_playouts(0.0); eng.set_gumbel(0, CV, CS)
    for first in (lambda: eng.set_root_noise(np.full((SLOTS, 43), 0.3, f32)), lambda: eng.set_forced_playouts(2.0)):
        first()
        with pytest.raises(P.AzrError) as e:
            eng.set_gumbel(4, CV, CS)
        assert e.value.code == 1 and "azr_mcts_set_gumbel" in str(e.value)
        eng.set_root_noise(None); eng.set_forced_playouts(0.0)
    # self-play: refused at the start, with a reason, and the handle goes on
    eng.selfplay_set_gumbel(4, CV, CS, GSEED)
    for on, off, word in ((lambda: eng.selfplay_set_dirichlet(0.3, 1), lambda: eng.selfplay_set_dirichlet(0.0), "Dirichlet"),
                          (lambda: eng.selfplay_set_playout_cap(0.5, 4, 1), lambda: eng.selfplay_set_playout_cap(1.0, 0), "playout cap"),
                          (lambda: eng.selfplay_set_forced_playouts(2.0), lambda: eng.selfplay_set_forced_playouts(0.0), "forced playouts")):
        on()
        with pytest.raises(P.AzrError) as e:
            eng.selfplay_start_games(BASE, 2)
        assert e.value.code == 1 and word in str(e.value) and "azr_selfplay_set_gumbel" in str(e.value)
        off()
    eng.selfplay_start_games(BASE, 2)
    eng.selfplay_run(4)
    assert eng.root_gumbel().any() and eng.counters()["errors"] == 0
    eng.close()
