"""GPU: a search budget and PUCT constant per side in the two-net arena (azr_arena_set_opponent_search).  Shapes of
tests/test_gpu_arena_mixed.py: 6 slots, 2 games per slot, nets of 1-2 blocks, max_game_rounds = 40.

  1. identity    player B set to the handle's own values plays what it played without the call
  2. the oracle  A = 12 simulations at hp 1.1 against B = 4 at hp 2.0, bit for bit against the composed oracle driver
                 (tests/arena_budget_ref.py, pinned to the oracle by tests/test_arena_budget_ref.py) with the two DEVICE nets called
                 back per evaluation; B = 9 at T = 2 (the S - S % T rule per side); B = 24 against A = 4 (the larger budget on B)
  3. role swap   the same pairing run from the other handle with the players' kinds exchanged plays the same games
  4. guards      S_B < T, a budget the node pool cannot hold, a call during an arena, the reset, self-play untouched

Without azr_arena_set_opponent_search every case fails at the missing symbol."""
import ctypes as C

import numpy as np
import pytest

import arena_budget_ref as R
import azr_testlib as T
from gpu_common import pkg

pytestmark = pytest.mark.gpu
FM = T.data_field_mask()
G, PER_SLOT, ROUNDS = 6, 2, 40


def run_arena(eng, k0, k1, total, cap, mirror, base):
    eng.arena_start(k0, k1, total, per_slot_cap=cap, mirror=mirror, base_seed=base)
    for _ in range(2000):
        if eng.arena_run(64):
            break
    else:
        raise AssertionError("arena did not finish")
    return eng.arena_results(), eng.arena_log()


def make_eval(eng):
    @T.EVAL_FN
    def f(ctx, in88, pi, v):
        x = np.ctypeslib.as_array(in88, shape=(88,)).copy()[None]
        p, vv = eng.predict(x)
        C.memmove(pi, p.ctypes.data, 43 * 4)
        v[0] = float(vv[0])
    return f


def six(res):
    return [res["count"], res["draw"], res["win"][0], res["win_and_started"][0], res["win"][1], res["win_and_started"][1]]


def pair(P, threads, sims_a=12, blocks=(1, 2), seeds=(31, 32), test_hooks=False, **kw):
    """the arena handle a (net A) and the opponent handle b (net B), both bf16"""
    a = P.Engine(G, blocks=blocks[0], sims=sims_a, dtype=P.NET_BF16, threads=threads, max_game_rounds=ROUNDS, test_hooks=test_hooks, **kw)
    b = P.Engine(G, blocks=blocks[1], sims=sims_a, dtype=P.NET_BF16, threads=threads, max_game_rounds=ROUNDS, test_hooks=test_hooks)
    a.set_weights(T.make_net_flat(blocks[0], seed=seeds[0], perturb_bn=True))
    b.set_weights(T.make_net_flat(blocks[1], seed=seeds[1], perturb_bn=True))
    a.arena_set_opponent(b)
    a.arena_collect_samples(True)
    return a, b


def everything(eng, k, mirror, base):
    """one arena; what a caller can see of it: results, log, the records' bytes (record order in the ring depends on which of the games
    that end in one pass is flushed first: sorted)"""
    res, (n, st, rd, fin) = run_arena(eng, k[0], k[1], 10 ** 6, PER_SLOT, mirror, base)
    c = eng.counters()
    assert (n == PER_SLOT).all() and c["errors"] == 0 and c["nodes_dropped"] == 0 and c["records_dropped"] == 0
    recs = eng.drain()
    assert len(recs) > 0
    # (the log's entries past a slot's last game are whatever the buffers held)
    return (six(res), n.copy(), st[:, :PER_SLOT].copy(), rd[:, :PER_SLOT].copy(), fin[:, :PER_SLOT].copy(),
            b"".join(sorted(r.tobytes() for r in recs)), c["simulations"])


def same(x, y):
    assert x[0] == y[0]
    for p, q in zip(x[1:5], y[1:5]):
        assert (p == q).all()
    assert x[5] == y[5] and x[6] == y[6]


# ---- 1. identity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mirror", ["sequential", "concurrent"])
def test_the_handles_own_values_change_nothing(mirror):
    P = pkg()
    mode = P.MIRROR_CONCURRENT if mirror == "concurrent" else P.MIRROR_SEQUENTIAL
    k = (P.PLAYER_ALPHAZERO, P.PLAYER_ALPHAZERO_B)
    a, b = pair(P, threads=2, sims_a=13)              # 13 at T = 2: both sides search 12
    before = everything(a, k, mode, 5200)
    a.arena_set_opponent_search(a.settings.mcts_simulations, a.settings.hp_exploration)
    same(everything(a, k, mode, 5200), before)
    a.arena_set_opponent_search(5, 3.0)
    other = everything(a, k, mode, 5200)
    assert other[5] != before[5]                      # ... and another budget does change the games
    a.arena_set_opponent_search()                     # None, None = the handle's own
    same(everything(a, k, mode, 5200), before)
    a.arena_set_opponent(None)
    a.close(); b.close()


# ---- 2. against the composed oracle driver --------------------------------------------------------------------------------------------
def against_the_oracle(P, threads, b_first, mirror, sims_a, hp_a, sims_b, hp_b, **kw):
    base = 5200
    a, b = pair(P, threads, sims_a=sims_a, hp_exploration=hp_a, **kw)
    a.arena_set_opponent_search(sims_b, hp_b)
    k = (P.PLAYER_ALPHAZERO_B, P.PLAYER_ALPHAZERO) if b_first else (P.PLAYER_ALPHAZERO, P.PLAYER_ALPHAZERO_B)
    mode = P.MIRROR_CONCURRENT if mirror == "concurrent" else P.MIRROR_SEQUENTIAL
    res, (n, st, rd, fin) = run_arena(a, k[0], k[1], 10 ** 6, PER_SLOT, mode, base)
    c = a.counters()
    print("counters", c)
    assert (n == PER_SLOT).all() and c["errors"] == 0 and c["nodes_dropped"] == 0 and c["records_dropped"] == 0
    recs = a.drain()

    ea, eb = make_eval(a), make_eval(b)
    cfg_a = T.default_settings(mcts_simulations=sims_a, hp_exploration=hp_a, mcts_threads=threads, max_game_rounds=ROUNDS)
    cfg_b = T.default_settings(mcts_simulations=sims_b, hp_exploration=hp_b, mcts_threads=threads, max_game_rounds=ROUNDS)
    tot = np.zeros(6, np.int64)
    blob = recs.tobytes()
    nrec = sims = 0
    for g in range(G):
        if mirror == "concurrent":
            o = R.play_half_games(k[0], k[1], PER_SLOT, g & 1, base + (g >> 1), G // 2, cfg_a, cfg_b, ea, eb)
        else:
            o = R.play_games(k[0], k[1], PER_SLOT, True, base + g, cfg_a, cfg_b, ea, eb)
        r6, ost, ord_, ofin, orec, osims = o
        assert (st[g, :PER_SLOT] == ost).all(), (g, st[g], ost)
        assert (rd[g, :PER_SLOT] == ord_).all(), g
        assert (fin[g, :PER_SLOT][:, FM] == ofin[:, FM]).all(), g
        tot += np.array(r6)
        sims += osims
        for gi, game in enumerate(orec):   # a finished game's records are flushed contiguously, z filled in
            assert len(game) > 0 and game.tobytes() in blob, (g, gi)
            nrec += len(game)
    assert nrec == len(recs)
    assert six(res) == list(tot)
    print("simulations: device", c["simulations"], "oracle drivers", sims)
    assert c["simulations"] == sims
    a.arena_set_opponent(None)
    a.close(); b.close()


@pytest.mark.parametrize("mirror", ["sequential", "concurrent"])
@pytest.mark.parametrize("b_first", [False, True])
@pytest.mark.parametrize("threads", [1, 2])
def test_budget_per_side_bit_exact_with_samples(orc, threads, b_first, mirror):
    """A = 12 simulations at hp 1.1, B = 4 at hp 2.0: statuses, rounds, final states, every (s, pi, z) record of both players, the six
    GameResults numbers and the simulation count against the oracle driver whose two players carry their own settings"""
    against_the_oracle(pkg(), threads, b_first, mirror, 12, 1.1, 4, 2.0)


def test_each_side_rounds_its_own_budget_down_to_the_threads(orc):
    """B = 9 at T = 2 searches 8 per decision while A searches 12: counters()['simulations'] is the oracle drivers' sum"""
    against_the_oracle(pkg(), 2, False, "sequential", 12, 1.1, 9, 2.0)


def test_the_larger_budget_on_side_b(orc):
    """B = 24 against A = 4: the pool is sized for B by the caller (node_capacity), nothing is dropped (asserted with the counters)"""
    against_the_oracle(pkg(), 2, True, "concurrent", 4, 1.1, 24, 2.0, node_capacity=16 * 25)


# ---- 3. role swap ---------------------------------------------------------------------------------------------------------------------
def game_blocks(recs):
    """the multiset of per-game record blocks of a drained ring.  A game's records are flushed as one block in decision order, and the
    round (bytes 44-45 of the record's NNInputData) never falls inside a game and starts at 0: a block ends where the round falls."""
    rounds = recs[:, 1 + 44].astype(np.int32) | (recs[:, 1 + 45].astype(np.int32) << 8)
    cuts = [0] + [i for i in range(1, len(recs)) if rounds[i] < rounds[i - 1]] + [len(recs)]
    return sorted(recs[a:b].tobytes() for a, b in zip(cuts[:-1], cuts[1:]))


@pytest.mark.parametrize("mirror,threads,counted", [("sequential", 1, False), ("concurrent", 2, True)])
def test_role_swap_plays_the_same_games(monkeypatch, mirror, threads, counted):
    """arena 1: handle X (12 simulations, net X) with opponent Y at (4, 2.0), players (AZ, AZ_B); arena 2: handle Y' (4 simulations,
    hp 2.0, net Y) with opponent X at (12, 1.1), players (AZ_B, AZ).  Player index 0 is net X at 12 simulations in both.  `counted`:
    in the test build under AZR_ARENA_COUNTED=2, where a silent drop to the read-back form is AZR_E_STATE."""
    P = pkg()
    if counted:
        monkeypatch.setenv("AZR_ARENA_COUNTED", "2")
    mode = P.MIRROR_CONCURRENT if mirror == "concurrent" else P.MIRROR_SEQUENTIAL
    base = 7300
    kw = dict(dtype=P.NET_BF16, threads=threads, max_game_rounds=ROUNDS, test_hooks=counted)
    wx, wy = T.make_net_flat(1, seed=51, perturb_bn=True), T.make_net_flat(2, seed=52, perturb_bn=True)

    def arena(h, opp, budget, kinds):
        h.arena_set_opponent(opp)
        h.arena_set_opponent_search(*budget)
        h.arena_collect_samples(True)
        res, (n, st, rd, fin) = run_arena(h, kinds[0], kinds[1], 10 ** 6, PER_SLOT, mode, base)
        c = h.counters()
        assert (n == PER_SLOT).all() and c["errors"] == 0 and c["nodes_dropped"] == 0
        out = six(res), st[:, :PER_SLOT].copy(), rd[:, :PER_SLOT].copy(), fin[:, :PER_SLOT].copy(), game_blocks(h.drain()), c["simulations"]
        h.arena_set_opponent(None)
        return out

    x = P.Engine(G, blocks=1, sims=12, **kw)
    y = P.Engine(G, blocks=2, sims=12, **kw)                                    # its own search settings are not read
    x.set_weights(wx); y.set_weights(wy)
    one = arena(x, y, (4, 2.0), (P.PLAYER_ALPHAZERO, P.PLAYER_ALPHAZERO_B))
    y2 = P.Engine(G, blocks=2, sims=4, hp_exploration=2.0, node_capacity=16 * 13, **kw)
    y2.set_weights(wy)
    two = arena(y2, x, (12, 1.1), (P.PLAYER_ALPHAZERO_B, P.PLAYER_ALPHAZERO))
    assert one[0] == two[0]
    for p, q in zip(one[1:4], two[1:4]):
        assert (p == q).all()
    assert len(one[4]) == G * PER_SLOT and one[4] == two[4]
    assert one[5] == two[5]
    x.close(); y.close(); y2.close()


# ---- 4. guards ------------------------------------------------------------------------------------------------------------------------
def test_guards():
    P = pkg()
    k = (P.PLAYER_ALPHAZERO, P.PLAYER_ALPHAZERO_B)
    a, b = pair(P, threads=2)                                                   # 12 simulations: a pool of 16 * 13 = 208 nodes
    before = everything(a, k, P.MIRROR_SEQUENTIAL, 5200)
    with pytest.raises(P.binding.AzrError) as e:
        a.arena_set_opponent_search(1, 2.0)                                     # S_B < T
    assert e.value.code == 1 and "mcts_threads" in str(e.value)                 # AZR_E_INVALID_ARGUMENT
    with pytest.raises(P.binding.AzrError) as e:
        a.arena_set_opponent_search(13, 2.0)                                    # 16 * 14 = 224 > 208
    assert e.value.code == 1 and "larger node_capacity" in str(e.value)
    a.arena_set_opponent_search(12, 2.0)                                        # the largest that fits
    # refused calls left the setting alone; (12, 2.0) is in force and holds over arena_start calls
    hp2 = everything(a, k, P.MIRROR_SEQUENTIAL, 5200)
    assert hp2[5] != before[5]
    same(everything(a, k, P.MIRROR_SEQUENTIAL, 5200), hp2)
    # between azr_arena_start and the finish
    a.arena_start(k[0], k[1], 10 ** 6, per_slot_cap=PER_SLOT, mirror=P.MIRROR_SEQUENTIAL, base_seed=5200)
    with pytest.raises(P.binding.AzrError) as e:
        a.arena_set_opponent_search(4, 2.0)
    assert e.value.code == 7                                                    # AZR_E_STATE
    assert not a.arena_run(1)
    with pytest.raises(P.binding.AzrError) as e:
        a.arena_set_opponent_search(4, 2.0)
    assert e.value.code == 7
    for _ in range(2000):
        if a.arena_run(64):
            break
    a.discard_samples()
    a.arena_set_opponent_search(4, 2.0)                                         # finished: accepted
    assert everything(a, k, P.MIRROR_SEQUENTIAL, 5200)[5] not in (before[5], hp2[5])
    # azr_arena_set_opponent_net(h, NULL) resets it
    a.arena_set_opponent(None)
    a.arena_set_opponent(b)
    same(everything(a, k, P.MIRROR_SEQUENTIAL, 5200), before)
    # a bad handle
    assert a.L.azr_arena_set_opponent_search(None, 4, 2.0) == 3                 # AZR_E_BAD_HANDLE
    a.arena_set_opponent(None)
    a.close(); b.close()


def test_self_play_never_reads_the_opponents_budget():
    """self-play on a handle whose player B has a budget of its own is byte-identical to self-play on a fresh handle"""
    P = pkg()

    def selfplay(set_budget):
        a = P.Engine(G, blocks=1, sims=4, dtype=P.NET_BF16, threads=2, max_game_rounds=12)   # short games: some finish in 1500 passes
        a.set_weights(T.make_net_flat(1, seed=31, perturb_bn=True))
        if set_budget:
            a.arena_set_opponent(a)
            a.arena_set_opponent_search(2, 2.0)
        a.selfplay_start(base_seed=99)
        a.selfplay_run(1500)
        c = a.counters()
        recs = a.drain()
        states = a.get_states()
        if set_budget:
            a.arena_set_opponent(None)
        a.close()
        return c, b"".join(sorted(r.tobytes() for r in recs)), states.tobytes()

    fresh, with_budget = selfplay(False), selfplay(True)
    assert fresh[0]["simulations"] > 0 and fresh[0]["games_finished"] > 0 and len(fresh[1]) > 0
    assert fresh == with_budget
