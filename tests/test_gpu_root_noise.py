"""GPU: root noise sampled per root (azr_mcts_set_root_noise, azr_selfplay_set_dirichlet, azr_mcts_root_noise,
azr_debug_root_noise).  The default stays the reference's constant DIR_NOISE_EPSI * DIR_NOISE_VALUE at every node
(alphazero_mcts.cpp:81); with a vector eta in force the first selection of every descent scores move m with
(1 - eps) P[m] + eps eta[m].  Checked here: the constant vector is today's search bit for bit (and the oracle's); the root formula
for a non-constant vector, pass by pass, against an fp32 restatement; depth 0 only; the game stream is not touched; the vector is a
function of (noise seed, game seed, decision, legal moves); the sampler is well-formed and is Dirichlet(alpha)."""
import ctypes as C

import numpy as np
import pytest

import azr_testlib as T
from azr_testlib import bits, host_stub_search
from gpu_common import pkg, setup_engine, stepped

pytestmark = pytest.mark.gpu
f32 = np.float32
FULL = (1 << 43) - 1


# ---- 1. the constant vector is today's search ------------------------------------------------------------------------------
def _two_decisions(orc, threads, eta_value, stub_name="orc_hash_eval"):
    """two consecutive decisions (the second search reuses the tree) of 8 new games; everything the search leaves behind"""
    stub = T.stub_fn(stub_name)
    P = pkg()
    G, sims = 8, 16
    eng = P.Engine(G, blocks=1, sims=sims, dtype=P.NET_F32, threads=threads)
    eng.new_games(np.arange(300, 300 + G, dtype=np.uint32))
    if eta_value is not None:
        eng.set_root_noise(np.full((G, 43), eta_value, f32))
        assert (eng.root_noise() == f32(eta_value)).all()
    else:
        eng.set_root_noise(None)
        assert (eng.root_noise() == 0).all()
    out = []
    for step in range(2):
        host_stub_search(eng, orc, stub)
        n, q, p = eng.root_stats()
        pi = eng.policy()
        mv = eng.pick(sample=False)
        assert (eng.make_moves(mv) == 0).all()
        out.append(dict(n=n, q=q, p=p, pi=pi, mv=mv, states=eng.get_states(), rng=eng.get_rng()))
    eng.close()
    return out


@pytest.mark.parametrize("threads", [1, 2])
def test_constant_vector_is_the_constant_search_and_the_oracles(orc, threads):
    constant_vector_is_the_oracles(orc, threads, "orc_hash_eval")


@pytest.mark.parametrize("threads", [1, 2])
def test_sharp_constant_vector_is_the_constant_search_and_the_oracles(orc, threads):
    """the same on the sharp stub: the mix (1 - eps) * P + eps * eta[m] on priors of exactly 0 and on denormal ones"""
    constant_vector_is_the_oracles(orc, threads, "orc_sharp_eval")


def constant_vector_is_the_oracles(orc, threads, stub_name):
    P = pkg()
    s = P.Settings()
    P.load_library().azr_default_settings(C.byref(s))
    a = _two_decisions(orc, threads, f32(s.dir_noise_value), stub_name)
    b = _two_decisions(orc, threads, None, stub_name)
    for step in range(2):
        for key in a[step]:
            assert a[step][key].tobytes() == b[step][key].tobytes(), (step, key)
    # ... and both are the oracle's search (the harness of test_gpu_mcts.py)
    evalfn = C.cast(T.stub_fn(stub_name), C.c_void_p)
    cfg = T.default_settings(mcts_simulations=16, mcts_threads=threads)
    d = np.zeros(160, np.uint8)
    for g in range(8):
        r, st = T.OrcRng(), T.OrcState()
        orc.orc_rng_seed(C.byref(r), 300 + g)
        orc.orc_new_game(C.byref(st), C.byref(r))
        m = orc.orc_mcts_create(C.byref(cfg))
        for step in range(2):
            n, q, p, pi = np.zeros(43, np.uint32), np.zeros(43, f32), np.zeros(43, f32), np.zeros(43, f32)
            assert orc.orc_mcts_simulate(m, C.byref(st), C.byref(r), evalfn, None) == 0
            orc.orc_mcts_root_stats(m, C.byref(st), T.ptr(n), T.ptr(q), T.ptr(p), None)
            orc.orc_mcts_policy(m, C.byref(st), T.ptr(pi))
            w = a[step]
            assert (n == w["n"][g]).all(), (step, g)
            for x, y in ((q, w["q"][g]), (p, w["p"][g]), (pi, w["pi"][g])):
                assert (x.view(np.uint32) == y.view(np.uint32)).all(), (step, g)
            mv = orc.orc_pick_highest(T.ptr(pi))
            assert mv == w["mv"][g]
            assert orc.orc_make_move(C.byref(st), mv, C.byref(r), C.byref(cfg)) == 0
            orc.orc_state_pack(C.byref(st), T.ptr(d))
            assert (d == w["states"][g]).all() and r.x == w["rng"][g], (step, g)
        orc.orc_mcts_destroy(m)


# ---- 2. the root formula, bit for bit ---------------------------------------------------------------------------------------
def puct_pick(orc, N, Q, Pr, valid, eta, eps, hp):
    """StateSimulations::getNextBestMoveAndSetVisited at the root with eps * eta[m] as the second term: np.float32 throughout,
    the operation order of tree_select; ties in unordered_map iteration order"""
    c1 = f32(1) - f32(eps)
    sumN = f32(int(N.sum()))
    noiseP = (c1 * Pr) + (f32(eps) * eta)
    v = (noiseP * f32(hp)) * np.sqrt(f32(1) + sumN)
    u = Q + v / (f32(1) + N.astype(f32))
    assert u.dtype == f32
    ok = bits(valid)
    best = u[ok].max()
    ties = [m for m in range(43) if ok[m] and u[m] == best]
    if len(ties) == 1:
        return ties[0]
    order = np.zeros(43, np.uint8)
    k = orc.orc_umap_order(int(valid), T.ptr(order))
    return [m for m in order[:k] if m in ties][0]


def test_root_formula_bit_for_bit_random_vector(orc):
    root_formula_random_vector(orc, False)


def test_sharp_root_formula_bit_for_bit_random_vector(orc):
    """the same on the sharp net of that seed: a random vector mixed into priors of exactly 0 and into denormal ones"""
    root_formula_random_vector(orc, True)


def root_formula_random_vector(orc, sharp):
    eng = setup_engine(24, sharp)
    valid = eng.valid_moves()
    r = np.random.default_rng(5).random((8, 43))
    eta = (r / r.sum(1, keepdims=True)).astype(f32)
    assert all(len(set(e)) == 43 for e in eta)   # no ties
    eps, hp = eng.settings.dir_noise_epsi, eng.settings.hp_exploration

    def check(i, prev, cur):
        for g in range(8):
            want = puct_pick(orc, prev[0][g], prev[1][g], prev[2][g], valid[g], eta[g], eps, hp)
            d = cur[0][g].astype(np.int64) - prev[0][g].astype(np.int64)
            assert d.sum() == 1 and d[want] == 1, (i, g, want, np.nonzero(d)[0])

    last = stepped(eng, eta, 24, check)
    assert (last[0].sum(1) == 24).all()
    assert (eng.root_noise() == eta).all()
    eng.close()


def test_root_formula_peaked_vector_is_visited_first(orc):
    eng = setup_engine(8)
    valid = eng.valid_moves()
    # the clean priors first (one search without noise), then 0.97 on the legal move with the lowest prior
    eng.set_root_noise(None)
    eng.simulate()
    prior = eng.root_stats()[2]
    eng.mcts_clear()
    eng.new_games(np.arange(4100, 4108, dtype=np.uint32))
    eta = np.zeros((8, 43), f32)
    low = []
    for g in range(8):
        ok = bits(valid[g])
        a = int(np.where(ok, prior[g], np.inf).argmin())
        assert prior[g][a] < 1.0 / ok.sum()
        eta[g][ok] = f32(0.03 / (ok.sum() - 1))
        eta[g][a] = f32(0.97)
        low.append(a)

    def check(i, prev, cur):
        if i == 0:
            for g in range(8):
                assert cur[0][g][low[g]] == 1 and cur[0][g].sum() == 1, g

    stepped(eng, eta, 1, check)
    eng.close()


# ---- 3. depth 0 only -----------------------------------------------------------------------------------------------------------
def test_noise_enters_the_first_selection_of_a_descent_only():
    P = pkg()
    G, sims = 8, 16
    eng = P.Engine(G, blocks=1, sims=sims, dtype=P.NET_F32, threads=1, dir_noise_epsi=1.0)
    eng.new_games(np.arange(70, 70 + G, dtype=np.uint32))
    valid = eng.valid_moves()
    a = np.array([int(v & -v).bit_length() - 1 for v in map(int, valid)], np.uint8)
    eta = np.zeros((G, 43), f32)
    eta[np.arange(G), a] = 1
    eng.set_root_noise(eta)
    rng = np.random.default_rng(9)
    eng.mcts_begin()
    for _ in range(sims + 4):
        x, need, act = eng.mcts_leaves()
        if act == 0:
            break
        pi = rng.random((G, 43)).astype(f32)
        eng.mcts_apply(pi / pi.sum(1, keepdims=True), rng.uniform(-0.05, 0.05, G).astype(f32))   # |Q| stays below the noise term
    assert eng.mcts_leaves()[2] == 0
    n = eng.root_stats()[0]
    assert (n[np.arange(G), a] == sims).all() and (n.sum(1) == sims).all()   # eps = 1, one-hot: the root visits `a` alone
    # the child reached through `a` was searched with the constant formula: (1 - eps) P + eps * DIR_NOISE_VALUE is the same for
    # every move there, so its 15 visits spread (with the one-hot vector applied below the root they would pile on one move)
    eng.set_root_noise(None)
    assert (eng.make_moves(a) == 0).all()
    nc = eng.root_stats()[0]
    assert (nc.sum(1) == sims - 1).all()
    assert ((nc > 0).sum(1) > 1).all(), nc
    eng.close()


# ---- 4. the game stream is untouched -------------------------------------------------------------------------------------------
def test_selfplay_game_stream_is_untouched_by_the_sampler():
    """eps = 0: the vector is drawn and mixed in with weight 0.  Had the sampler taken anything from the games' RNG streams, or
    the noise path rounded differently, dice, deals or sampled moves would move."""
    P = pkg()
    G = 16
    flat = T.make_net_flat(1, seed=11, perturb_bn=True)
    got = []
    for alpha in (0.0, 0.3):
        eng = P.Engine(G, blocks=1, sims=4, dtype=P.NET_F32, threads=2, dir_noise_epsi=0.0)
        eng.set_weights(flat)
        eng.selfplay_set_dirichlet(alpha, 77)
        eng.selfplay_start(9000)
        eng.selfplay_run(40)
        noise = eng.root_noise()
        got.append((eng.drain().tobytes(), eng.get_states().tobytes(), eng.get_rng().tobytes(), eng.counters()))
        assert (noise == 0).all() if alpha == 0 else (np.abs(noise.astype(np.float64).sum(1) - 1) <= 1e-6).all()
        eng.close()
    assert got[0][3]["decisions"] > G
    for x, y in zip(got[0], got[1]):
        assert x == y


# ---- 5. the vector is a function of the seeds ------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", [1, 2])
def test_selfplay_vectors_are_a_function_of_the_seeds(threads):
    P = pkg()
    alpha, nseed, base = 0.3, 1234, 5000
    flat = T.make_net_flat(1, seed=11, perturb_bn=True)
    first = {}
    for G in (8, 16):
        eng = P.Engine(G, blocks=1, sims=8, dtype=P.NET_F32, threads=threads)
        eng.set_weights(flat)
        eng.selfplay_set_dirichlet(alpha, nseed)
        eng.selfplay_start(base)
        seeds = np.arange(base, base + G, dtype=np.uint32)   # Ctl.seed of every slot's first game
        eta = eng.root_noise()
        want = eng.debug_root_noise(alpha, nseed, seeds, np.zeros(G, np.uint32), eng.valid_moves())
        assert (eta.view(np.uint32) == want.view(np.uint32)).all()
        assert (np.abs(eta.astype(np.float64).sum(1) - 1) <= 1e-6).all()
        first[G] = eta
        eng.selfplay_run(30)
        c = eng.counters()
        assert c["games_finished"] == 0 and c["errors"] == 0 and c["decisions"] >= G   # every slot still plays its first game
        eta = eng.root_noise()
        valid = eng.valid_moves()
        # Ctl.decisions is not exposed: the decision index of each game is the one whose vector this is, and the indices add up to
        # the decisions the engine counted
        D = 64
        total = 0
        for g in range(G):
            cand = eng.debug_root_noise(alpha, nseed, np.full(D, seeds[g], np.uint32), np.arange(D, dtype=np.uint32), np.full(D, valid[g], np.uint64))
            hit = [d for d in range(D) if (cand[d].view(np.uint32) == eta[g].view(np.uint32)).all()]
            assert len(hit) == 1, (g, hit)
            total += hit[0]
        assert total == c["decisions"]
        other = eng.debug_root_noise(alpha, nseed + 1, seeds, np.zeros(G, np.uint32), np.full(G, FULL, np.uint64))
        same = eng.debug_root_noise(alpha, nseed, seeds, np.zeros(G, np.uint32), np.full(G, FULL, np.uint64))
        assert not (other == same).all(1).any()
        eng.close()
    assert (first[8] == first[16][:8]).all()   # not of the number of games


def test_argument_errors():
    P = pkg()
    eng = P.Engine(2, blocks=1, sims=2, dtype=P.NET_F32)
    L = eng.L
    assert L.azr_selfplay_set_dirichlet(None, 0.3, 1) == 3 and L.azr_mcts_set_root_noise(None, None) == 3      # AZR_E_BAD_HANDLE
    assert L.azr_mcts_root_noise(None, None) == 3 and L.azr_debug_root_noise(None, 0.3, 1, None, None, None, 0, None) == 3
    for bad in (float("nan"), 10.5):
        assert L.azr_selfplay_set_dirichlet(eng.h, bad, 1) == 1                                                  # AZR_E_INVALID_ARGUMENT
        with pytest.raises(P.AzrError):
            eng.debug_root_noise(bad, 1, [1], [0], [FULL])
    eng.selfplay_set_dirichlet(10.0, 1)
    eng.selfplay_set_dirichlet(-1.0, 1)   # off
    eng.close()


# ---- 6. the sampler is well-formed ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sampler():
    P = pkg()
    eng = P.Engine(1, blocks=1, sims=1, dtype=P.NET_F32, node_capacity=64)
    yield eng
    eng.close()


MASKS = [1 << 42, (1 << 5) | (1 << 42), sum(1 << i for i in (0, 3, 7, 11, 19, 23, 30, 37, 41, 42)), FULL]


@pytest.mark.parametrize("alpha", [0.03, 0.3, 1.0, 10.0])
def test_sampler_well_formed(sampler, alpha):
    n = 1024
    for mask in MASKS:
        ok = bits(mask)
        eta = sampler.debug_root_noise(alpha, 3, np.full(n, 42, np.uint32), np.arange(n, dtype=np.uint32), np.full(n, mask, np.uint64))
        assert np.isfinite(eta).all() and (eta >= 0).all()
        assert (eta[:, ~ok] == 0).all()
        assert (np.abs(eta.astype(np.float64).sum(1) - 1) <= 1e-6).all()
        if ok.sum() == 1:
            assert (eta[:, ok] == 1.0).all()
        elif alpha >= 1:   # (below 1 a draw can round to a corner of the simplex, and corners repeat)
            assert len(np.unique(eta, axis=0)) == n   # every decision its own vector


# ---- 7. the sampler is Dirichlet(alpha) ------------------------------------------------------------------------------------------
def beta_moment(alpha, k, j):
    """E[eta^j] of one coordinate of a symmetric Dirichlet(alpha) over k moves"""
    m = 1.0
    for i in range(j):
        m *= (alpha + i) / (k * alpha + i)
    return m


@pytest.mark.parametrize("alpha,k", [(0.3, 10), (1.0, 4)])
def test_sampler_is_dirichlet(sampler, alpha, k):
    """every bound is 6 standard errors, the standard errors from the closed forms or from 10^6 numpy draws, never from the
    samples under test: ~150 checks, false-alarm rate below 1e-6"""
    n = 8192
    lanes = [0, 3, 7, 11, 19, 23, 30, 37, 41, 42][10 - k:]
    mask = sum(1 << i for i in lanes)
    eta = sampler.debug_root_noise(alpha, 99, np.full(n, 17, np.uint32), np.arange(n, dtype=np.uint32),   # consecutive decisions of one game
                                   np.full(n, mask, np.uint64)).astype(np.float64)[:, lanes]
    m1, m2, m4 = (beta_moment(alpha, k, j) for j in (1, 2, 4))
    se1, se2 = np.sqrt((m2 - m1 * m1) / n), np.sqrt((m4 - m2 * m2) / n)
    ref = np.random.default_rng(2026).dirichlet(np.full(k, alpha), 10 ** 6)
    for i in range(k):
        x = eta[:, i]
        print("lane %d: mean %+.2f se, mean of squares %+.2f se" % (lanes[i], (x.mean() - m1) / se1, ((x * x).mean() - m2) / se2))
        assert abs(x.mean() - m1) <= 6 * se1, (i, x.mean(), m1, se1)
        assert abs((x * x).mean() - m2) <= 6 * se2, (i, (x * x).mean(), m2, se2)
        for t in (0.01, 0.1, 0.5):
            pg, pr = (x < t).mean(), (ref[:, i] < t).mean()
            p = ((x < t).sum() + (ref[:, i] < t).sum()) / (n + len(ref))
            sd = np.sqrt(p * (1 - p) * (1.0 / n + 1.0 / len(ref)))
            assert abs(pg - pr) <= 6 * sd, (i, t, pg, pr, sd)
        r = np.corrcoef(x[:-1], x[1:])[0, 1]   # lag 1 over consecutive decisions
        assert abs(r) <= 6 / np.sqrt(n), (i, r)
    cross = alpha * alpha / (k * alpha * (k * alpha + 1))
    se = (ref[:, 0] * ref[:, 1]).std() / np.sqrt(n)
    assert abs((eta[:, 0] * eta[:, 1]).mean() - cross) <= 6 * se
