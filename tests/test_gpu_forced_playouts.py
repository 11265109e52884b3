"""GPU: forced playouts and policy target pruning at the root (azr_mcts_set_forced_playouts, azr_mcts_pruned_policy,
azr_selfplay_set_forced_playouts).  The contract is include/azr.h's; tests/forced_playouts_ref.py restates it in np.float32.  Checked
here: the root rule pass by pass, bit for bit; off is the engine that never called the setter; depth 0 only; the pruned counts and
policy against the restatement over three decisions with tree reuse; device self-play against the same games retraced decision by
decision through the host-stepped entry points (with and without a playout cap, with and without Dirichlet noise), and against itself
with pruning off; argument checks.
Engines of 8 games, one block, NET_F32."""
import os

import numpy as np
import pytest

import azr_testlib as T
import forced_playouts_ref as F
import playout_cap_ref as R
from gpu_common import pkg
from test_gpu_root_noise import _setup_engine, _stepped

pytestmark = pytest.mark.gpu
f32 = np.float32
G = 8


def _bitwise(a, b):
    return a.tobytes() == b.tobytes()


# ---- 1. the root rule, bit for bit -----------------------------------------------------------------------------------------------
def test_root_rule_bit_for_bit(orc):
    eng = _setup_engine(32)
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

    last = _stepped(eng, eta, 32, check)
    assert (last[0].sum(1) == 32).all()
    print("passes where the forced pick is not PUCT's, per game:", differs)
    assert (differs > 0).sum() >= G // 2, differs
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
        eng = _setup_engine(32)
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
    eng = _setup_engine(32)
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
    eng = _setup_engine(32)
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


def _late_positions():
    """four running positions 20 and 10 moves before the end of golden games that reach the last rounds: the games end soon"""
    gold = np.load(os.path.join(T.GOLDEN, "rules_games.npz"))
    ends = gold["starts"][1:]
    idx = [ends[3] - 20, ends[13] - 20, ends[19] - 20, ends[3] - 10]
    states = np.concatenate([gold["states"][idx], gold["states"][idx]]).copy()   # slots 4..7 idle under the quota
    return states, np.arange(600, 600 + G, dtype=np.uint32)


def _selfplay(threads, cap, prune, alpha=ALPHA):
    """alpha = 0: azr_selfplay_set_dirichlet is never called (forced playouts in force, no Dirichlet noise set)"""
    P = pkg()
    eng = P.Engine(G, blocks=1, sims=SIMS, dtype=P.NET_F32, threads=threads)
    eng.set_weights(T.make_net_flat(1, seed=11, perturb_bn=True))
    states, rngs = _late_positions()
    eng.set_states(states)
    eng.set_rng(rngs)
    if alpha:
        eng.selfplay_set_dirichlet(alpha, NSEED)
    eng.selfplay_set_forced_playouts(K, prune)
    if cap:
        eng.selfplay_set_playout_cap(0.5, FAST, CSEED)
    eng.selfplay_start_games_from_states(BASE, QUOTA)
    recs = []
    for _ in range(400):
        eng.selfplay_run(64)
        assert alpha or not eng.root_noise().any()                # no Dirichlet noise in force: azr_mcts_root_noise reads zeros
        recs.append(eng.drain())
        c = eng.counters()
        if c["games_finished"] + c["errors"] >= QUOTA:
            break
    c = eng.counters()
    assert c["games_finished"] == QUOTA and c["errors"] == 0 and c["nodes_dropped"] == 0 and c["records_dropped"] == 0, c
    eng.close()
    return np.concatenate(recs), c


def _retrace(threads, cap, alpha=ALPHA):
    """the same four games through azr_mcts_*: per decision the kind by the cap's coin, the vector of azr_debug_root_noise (or the
    constant: a fast decision, and every decision with alpha = 0), the factor and the budget of that kind, one search, the pruned
    policy into the record, the unpruned pick as the move"""
    P = pkg()
    eng = P.Engine(G, blocks=1, sims=SIMS, dtype=P.NET_F32, threads=threads)
    eng.set_weights(T.make_net_flat(1, seed=11, perturb_bn=True))
    states, rngs = _late_positions()
    dnv, thr = f32(eng.settings.dir_noise_value), eng.settings.temperature_threshold
    games, tot = [], dict(decisions=0, simulations=0, samples=0)
    for g in range(QUOTA):
        eng.set_states(np.repeat(states[g:g + 1], G, 0))          # every slot retraces game g; slot 0 is read
        eng.set_rng(np.full(G, rngs[g], np.uint32))
        eng.mcts_clear()
        recs, d = [], 0
        while True:
            full = R.coin(0.5, CSEED, BASE + g, d) if cap else True
            valid = eng.valid_moves()
            eta = eng.debug_root_noise(alpha, NSEED, [BASE + g], [d], valid[:1]) if full and alpha else np.full((1, 43), dnv, f32)
            eng.set_root_noise(np.repeat(eta, G, 0))
            eng.set_forced_playouts(K if full else 0.0)
            eng.set_simulations(SIMS if full else FAST)
            eng.simulate()
            st = eng.get_states()[0]
            ppi = eng.pruned_policy()[0][0]
            mv = eng.pick(sample=not (int(st[144]) + 256 * int(st[145]) > thr))
            if full:
                rec = np.zeros(265, np.uint8)
                rec[0] = st[146]
                rec[1:89] = eng.encode()[0]
                rec[93:265] = ppi.view(np.uint8)
                recs.append(rec)
            assert (eng.make_moves(mv) == 0).all()
            budget = SIMS if full else FAST
            d += 1; tot["decisions"] += 1; tot["simulations"] += budget - budget % threads; tot["samples"] += int(full)
            status = int(eng.status()[0])
            if status != -1:
                break
            assert d < 2000
        for rec in recs:
            z = 0.0 if status == -2 else (1.0 if int(rec[0]) == status else -1.0)
            rec[89:93] = np.array([z], f32).view(np.uint8)
        games.append(np.array(recs, np.uint8).reshape(len(recs), 265))
    eng.close()
    return games, tot


def _check_composition(threads, cap, alpha):
    recs, c = _selfplay(threads, cap, True, alpha)
    games, tot = _retrace(threads, cap, alpha)
    print("decisions per game:", [len(g) for g in games], tot)
    blob = recs.tobytes()
    for g, want in enumerate(games):
        assert len(want) > 0 and want.tobytes() in blob, f"game {g}: its record stream is not in the device's output"
    assert len(recs) == sum(len(g) for g in games)
    assert {k: c[k] for k in tot} == tot
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
