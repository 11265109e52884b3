"""GPU: forced playouts and policy target pruning at the root (azr_mcts_set_forced_playouts, azr_mcts_pruned_policy,
azr_selfplay_set_forced_playouts).  The contract is include/azr.h's; tests/forced_playouts_ref.py restates it in np.float32.  Checked
here: the root rule pass by pass, bit for bit; off is the engine that never called the setter; depth 0 only; the pruned counts and
policy against the restatement over three decisions with tree reuse; device self-play against the same games retraced decision by
decision through the host-stepped entry points (with and without a playout cap, with and without Dirichlet noise), and against itself
with pruning off; argument checks.
Engines of 8 games, one block, NET_F32."""
import numpy as np
import pytest

import azr_testlib as T
import forced_playouts_ref as F
import selfplay_retrace as SR
from gpu_common import pkg, setup_engine, stepped

pytestmark = pytest.mark.gpu
f32 = np.float32
G = 8


def _bitwise(a, b):
    return a.tobytes() == b.tobytes()


# ---- 1. the root rule, bit for bit -----------------------------------------------------------------------------------------------
def test_root_rule_bit_for_bit(orc):
    root_rule(orc, False)


def test_sharp_root_rule_bit_for_bit(orc):
    """the same on the sharp net of that seed: priors of exactly 0 (the threshold sqrt(k * noiseP * sumN) rests on the noise term alone),
    denormal priors and values of +-1.  How often the forced pick differs from PUCT's is printed, not required."""
    root_rule(orc, True)


def root_rule(orc, sharp):
    eng = setup_engine(32, sharp)
    valid = eng.valid_moves()
    r = np.random.default_rng(5).random((G, 43))
    eta = (r / r.sum(1, keepdims=True)).astype(f32)
    assert all(len(set(e)) == 43 for e in eta)   # no ties
    eps, hp, k = eng.settings.dir_noise_epsi, eng.settings.hp_exploration, 8.0
    eng.set_forced_playouts(k)
    differs = np.zeros(G, int)

    def check(i, prev, cur):
        for g in range(G):
            order = lambda: F.umap_order(orc, valid[g])
            want = F.forced_pick(prev[0][g], prev[1][g], prev[2][g], valid[g], eta[g], eps, hp, k, order)
            plain = F.puct_pick(prev[0][g], prev[1][g], prev[2][g], valid[g], eta[g], eps, hp, order)
            d = cur[0][g].astype(np.int64) - prev[0][g].astype(np.int64)
            assert d.sum() == 1 and d[want] == 1, (i, g, want, plain, np.nonzero(d)[0])
            differs[g] += int(want != plain)

    last = stepped(eng, eta, 32, check)
    assert (last[0].sum(1) == 32).all()
    print("passes where the forced pick is not PUCT's, per game:", differs)
    assert sharp or (differs > 0).sum() >= G // 2, differs
    if sharp:
        prior = last[2]
        zero = sum(int((prior[g][T.bits(valid[g])] == 0).any()) for g in range(G))
        print("sharp roots: zero legal prior rows %d, rows with a zero prior on a legal move %d" % ((prior == 0).all(1).sum(), zero))
        assert zero > 0   # the condition of the case: the threshold is taken at P == 0
    eng.close()


# ---- 2. off is the parent --------------------------------------------------------------------------------------------------------
def _two_decisions(threads, call):
    P = pkg()
    eng = P.Engine(G, blocks=1, sims=16, dtype=P.NET_F32, threads=threads)
    eng.set_weights(T.make_net_flat(1, seed=23, perturb_bn=True))
    eng.new_games(np.arange(300, 300 + G, dtype=np.uint32))
    if call:
        eng.set_forced_playouts(0.0)
    out = []
    for step in range(2):
        eng.simulate()
        n, q, p = eng.root_stats()
        pi = eng.policy()
        if call:
            ppi, pn = eng.pruned_policy()
            assert _bitwise(ppi, pi) and (pn == n).all()          # no factor in force: N' = N
        mv = eng.pick(sample=step == 1)
        assert (eng.make_moves(mv) == 0).all()
        out.append(dict(n=n, q=q, p=p, pi=pi, mv=mv, states=eng.get_states(), rng=eng.get_rng()))
    eng.close()
    return out


@pytest.mark.parametrize("threads", [1, 2])
def test_off_is_the_engine_that_never_called_it(threads):
    a, b = _two_decisions(threads, False), _two_decisions(threads, True)
    for step in range(2):
        assert a[step]["n"].sum() > 0
        for key in a[step]:
            assert _bitwise(a[step][key], b[step][key]), (step, key)


def test_without_a_vector_forcing_runs_on_the_constant_form():
    """no root vector set: nf is computed from (1 - eps) P + eps * DIR_NOISE_VALUE, the same search and pruning as under the vector
    that holds DIR_NOISE_VALUE in every entry"""
    got = []
    for vector in (False, True):
        eng = setup_engine(32)
        if vector:
            eng.set_root_noise(np.full((G, 43), eng.settings.dir_noise_value, f32))
        eng.set_forced_playouts(2.0)
        eng.simulate()
        n, q, p = eng.root_stats()
        ppi, pn = eng.pruned_policy()
        got.append((n, q, p, ppi, pn, eng.get_rng()))
        eng.close()
    assert (got[0][0].sum(1) == 32).all()
    for x, y in zip(*got):
        assert _bitwise(x, y)
    # ... and it is not the unforced search
    eng = setup_engine(32)
    eng.simulate()
    assert (eng.root_stats()[0] != got[0][0]).any()
    eng.close()


# ---- 3. depth 0 only -------------------------------------------------------------------------------------------------------------
def test_forcing_acts_on_the_first_selection_of_a_descent_only():
    """eps = 1 and eta = 0: noiseP is 0 at the root, so nf = 0 there and nothing can be forced; below the root noiseP is the constant
    DIR_NOISE_VALUE > 0, where a leaked rule would force every tried move (nf = sqrt(8 * 0.3 * sumN): 3.1 after four visits).  With
    noiseP = 0 the root's score is Q alone, so the 64 descents try the legal moves once each and then stay with the best values: the
    most visited move's child is a searched node in (at least) half of the games, which the test asserts before it compares."""
    P = pkg()
    got = []
    for k in (0.0, 8.0):
        eng = P.Engine(G, blocks=1, sims=64, dtype=P.NET_F32, threads=1, dir_noise_epsi=1.0)
        eng.set_weights(T.make_net_flat(1, seed=23, perturb_bn=True))
        eng.new_games(np.arange(4100, 4100 + G, dtype=np.uint32))
        eng.set_root_noise(np.zeros((G, 43), f32))
        eng.set_forced_playouts(k)
        eng.simulate()
        n, q, _ = eng.root_stats()
        assert (n.sum(1) == 64).all()
        mv = n.argmax(1).astype(np.uint8)
        assert (eng.make_moves(mv) == 0).all()
        nc, qc, _ = eng.root_stats()
        print("k = %g: visits of the most visited move" % k, n.max(1), "visits below it", nc.sum(1))
        assert ((nc.sum(1) >= 4).sum() >= G // 2), (nc.sum(1), n.max(1))   # the child was searched
        got.append((n, q, nc, qc))
        eng.close()
    for x, y in zip(*got):
        assert _bitwise(x, y)


# ---- 4. pruning against the restatement ----------------------------------------------------------------------------------------------
def test_pruned_policy_against_the_restatement_over_three_decisions():
    eng = setup_engine(32)
    eps, hp, k = eng.settings.dir_noise_epsi, eng.settings.hp_exploration, 2.0
    eng.set_forced_playouts(k)
    rng = np.random.default_rng(8)
    changed = 0
    for step in range(3):
        valid = eng.valid_moves()
        eta = np.zeros((G, 43), f32)
        for g in range(G):                                        # a peaked vector: 0.97 on one legal move
            ok = F.bits(valid[g])
            a = int(rng.choice(np.nonzero(ok)[0]))
            eta[g][ok] = f32(0.03 / max(ok.sum() - 1, 1))
            eta[g][a] = f32(0.97) if ok.sum() > 1 else f32(1)
        eng.set_root_noise(eta)
        eng.simulate()
        n, q, p = eng.root_stats()
        pi, (ppi, pn) = eng.policy(), eng.pruned_policy()
        mv = eng.pick(sample=False)
        if step:
            assert (n.sum(1) >= 32).all() and (n.sum(1) > 32).sum() >= G // 2, n.sum(1)   # roots that carry the previous search's visits
        for g in range(G):
            want_n = F.prune_counts(n[g], q[g], p[g], valid[g], eta[g], eps, hp, k)
            assert (pn[g] == want_n).all(), (step, g, n[g], pn[g], want_n)
            assert _bitwise(ppi[g], F.root_policy(want_n, valid[g])), (step, g)
            assert _bitwise(pi[g], F.root_policy(n[g], valid[g])), (step, g)        # azr_mcts_policy is the unpruned one
            assert mv[g] == int(np.argmax(pi[g])) and pi[g][mv[g]] > 0, (step, g)   # the move comes from N (strict >, lowest index)
            changed += int((pn[g] != n[g]).any())
        assert (eng.make_moves(mv) == 0).all()
    print("roots whose pruned counts differ from N: %d of %d" % (changed, 3 * G))
    assert changed >= 3 * G // 2
    eng.close()


# ---- 5. self-play equals the host-stepped composition -------------------------------------------------------------------------------
BASE, NSEED, CSEED, SIMS, FAST, ALPHA, K, QUOTA = 9100, 77, 99, 16, 4, 0.3, 2.0, 4


def _run(threads, cap, prune, alpha=ALPHA):
    """alpha = 0: azr_selfplay_set_dirichlet is never called (forced playouts in force, no Dirichlet noise set)"""
    return SR.Run(BASE, QUOTA, threads, SIMS, fast=FAST, cap=(0.5, CSEED) if cap else None, dirichlet=(alpha, NSEED) if alpha else None,
                  forced=(K, prune))


def _selfplay(threads, cap, prune, alpha):
    def no_noise(i, eng):
        assert alpha or not eng.root_noise().any()                # no Dirichlet noise in force: azr_mcts_root_noise reads zeros

    eng = SR.selfplay(_run(threads, cap, prune, alpha))
    out = SR.play_out(eng, QUOTA, 64, 400, after_run=no_noise)
    eng.close()
    return out


def _check_composition(threads, cap, alpha):
    recs, c = _selfplay(threads, cap, True, alpha)
    games, tot = SR.retrace(_run(threads, cap, True, alpha))
    print("decisions per game:", [len(g.records) for g in games], tot)
    SR.assert_streams(recs, c, [(g.records, None) for g in games], tot)
    assert c["samples"] == tot["samples"]
    # pruning off: the same games, the same records outside pi
    plain, c0 = _selfplay(threads, cap, False, alpha)
    assert c0 == c and plain.shape == recs.shape
    assert (plain[:, :93] == recs[:, :93]).all()
    differ = (plain[:, 93:] != recs[:, 93:]).any(1)
    print("records whose pi pruning changed: %d of %d" % (differ.sum(), len(recs)))
    assert differ.any()


@pytest.mark.parametrize("threads,cap", [(1, False), (2, False), (2, True)])
def test_selfplay_is_the_host_stepped_composition(threads, cap):
    _check_composition(threads, cap, ALPHA)


@pytest.mark.parametrize("threads,cap", [(2, False), (2, True)])
def test_selfplay_without_dirichlet_is_the_host_stepped_composition(threads, cap):
    """forced playouts in force, azr_selfplay_set_dirichlet never called: every root, full or fast, runs on the constant vector"""
    _check_composition(threads, cap, 0.0)


# ---- 6. argument errors ------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    P = pkg()
    eng = P.Engine(2, blocks=1, sims=4, dtype=P.NET_F32, threads=2)
    L = eng.L
    assert L.azr_mcts_set_forced_playouts(None, 2.0) == 3 and L.azr_selfplay_set_forced_playouts(None, 2.0, 0) == 3   # AZR_E_BAD_HANDLE
    assert L.azr_mcts_pruned_policy(None, None, None) == 3
    for bad in (float("nan"), 8.5):
        for call, name in ((lambda: eng.set_forced_playouts(bad), "azr_mcts_set_forced_playouts"),
                           (lambda: eng.selfplay_set_forced_playouts(bad, False), "azr_selfplay_set_forced_playouts")):
            with pytest.raises(P.AzrError) as e:
                call()
            assert e.value.code == 1 and name in str(e.value), (bad, name)
    for k in (0.0, -1.0):
        with pytest.raises(P.AzrError) as e:
            eng.selfplay_set_forced_playouts(k, True)             # pruning without forcing
        assert e.value.code == 1 and "azr_selfplay_set_forced_playouts" in str(e.value)
    for bad in (1, 5):                                            # below the thread count, above mcts_simulations
        with pytest.raises(P.AzrError) as e:
            eng.set_simulations(bad)
        assert e.value.code == 1 and "azr_mcts_set_simulations" in str(e.value)
    eng.set_forced_playouts(8.0); eng.set_forced_playouts(-3.0)
    eng.selfplay_set_forced_playouts(8.0, True); eng.selfplay_set_forced_playouts(0.0, False)
    eng.set_simulations(2); eng.set_simulations(0)
    assert L.azr_mcts_pruned_policy(eng.h, None, None) == 1
    eng.close()
