"""An arena and its host-stepped retrace (TEST INFRASTRUCTURE, not collected): the proof of the arena's search settings per side
(azr_arena_set_gumbel) where the oracle has no such search.  The arena plays one pair of games per slot, AZR_MIRROR_OFF with a slot cap
of 1 (a slot takes games from the quota two at a time): slot g's first game is new_games([base + g]) with player 0 to move, its second
a fresh deal from the slot's RNG stream where the first game left it — new_games([that RNG word]): a stream's word seeds itself — with
player 1 to move.  The retrace plays the same games one after the other on host-stepped handles of one slot: the handle of the player
to move carries that side's net, PUCT constant, budget and search (azr_mcts_set_gumbel, _set_gumbel_tree, _set_root_gumbel(NULL),
_set_simulations); state and RNG word travel with get_states / set_states and get_rng / set_rng; azr_mcts_clear at a turn's first decision, where the arena's two trims in a row leave an empty tree, and nothing but
azr_mcts_simulate's own trim inside a turn; then azr_mcts_gumbel_pick — or azr_mcts_pick(sample = 0) on a PUCT side — and make_moves.
Engines of NET_F32, the weights of make_net_flat(blocks, seed, perturb_bn=True).
A Shape is the slots and max_game_rounds of a run.  A round is one player's turn; the setup phase is 26 turns of two decisions each (an
army for the mover, one for the neutral player), every root of it with 14 or so legal moves, and only then come the turns that attack,
whose mobilisation roots have two legal moves.  A host-stepped decision costs about 10 ms, so SHORT (4 slots = 8 games, 12 rounds, 24
decisions a game) stays inside the setup phase, and LONG (2 slots = 4 games, 28 rounds: two turns past the setup) reaches the rest."""
from typing import NamedTuple

import numpy as np

import azr_testlib as T

f32 = np.float32
PER_SLOT = 2
CV, CS = 50.0, 0.5
FM = T.data_field_mask()


class Shape(NamedTuple):
    slots: int
    rounds: int


SHORT, LONG = Shape(4, 12), Shape(2, 28)


class Side(NamedTuple):
    """one AlphaZero player: its budget as given (the engine searches sims - sims % T), its PUCT constant, its Gumbel search (m = 0:
    PUCT) and its net"""
    sims: int
    hp: float = 1.1
    m: int = 0
    tree: int = 0
    blocks: int = 1
    seed: int = 31


class Game(NamedTuple):
    """one retraced game: the player that started it, its records with z filled in [n, 265], the final state [160], status, round count,
    simulations, and per decision (the sum of the root's N row when its search began, the number of legal moves, the mover's m)"""
    start: int
    records: np.ndarray
    final: np.ndarray
    status: int
    rounds: int
    simulations: int
    decisions: list


def engine(P, side, threads, slots, rounds, **kw):
    eng = P.Engine(slots, blocks=side.blocks, sims=side.sims, dtype=P.NET_F32, threads=threads, hp_exploration=side.hp, max_game_rounds=rounds, **kw)
    eng.set_weights(T.make_net_flat(side.blocks, seed=side.seed, perturb_bn=True))
    return eng


def arena_engines(P, a, b, threads, shape, one_net=False):
    """the arena handle (side a's net and settings, node pools for the larger budget) with its opponent attached: a handle of side b's
    net, or — one_net — itself"""
    eng = engine(P, a, threads, *shape, node_capacity=16 * (max(a.sims, b.sims) + 1))
    opp = eng if one_net else engine(P, b._replace(sims=a.sims), threads, *shape)
    eng.arena_set_opponent(opp)
    return eng, opp


def close(eng, opp):
    eng.arena_set_opponent(None)
    eng.close()
    if opp is not eng:
        opp.close()


def configure(P, eng, a, b):
    """what the arena handle is told before its start: player B's budget and PUCT constant, both sides' search"""
    eng.arena_set_opponent_search(b.sims, b.hp)
    eng.arena_set_gumbel(P.PLAYER_ALPHAZERO, a.m, CV, CS, a.tree)
    eng.arena_set_gumbel(P.PLAYER_ALPHAZERO_B, b.m, CV, CS, b.tree)


def play(eng, kinds, base, collect=True):
    """one arena of one pair of games per slot, and what a caller can see of it: the six result numbers, the log's two games per slot
    (status, rounds, final state under the data mask), the records' bytes (sorted: the order in the ring depends on which of the games that end
    in one pass is flushed first) and the counters"""
    P, slots = __import__("gpu_common").pkg(), eng.G
    eng.arena_collect_samples(collect)
    eng.arena_start(kinds[0], kinds[1], 10 ** 6, per_slot_cap=1, mirror=P.MIRROR_OFF, base_seed=base)
    for _ in range(2000):
        if eng.arena_run(64):
            break
    else:
        raise AssertionError("arena did not finish")
    r, (n, st, rd, fin) = eng.arena_results(), eng.arena_log()
    c = eng.counters()
    assert (n == PER_SLOT).all() and c["errors"] == 0 and c["nodes_dropped"] == 0 and c["records_dropped"] == 0, (n, c)
    recs = eng.drain() if collect else np.zeros((0, 265), np.uint8)
    six = [r["count"], r["draw"], r["win"][0], r["win_and_started"][0], r["win"][1], r["win_and_started"][1]]
    return (six, st[:slots, :PER_SLOT].astype(int).ravel().tolist(), rd[:slots, :PER_SLOT].astype(int).ravel().tolist(),
            fin[:slots, :PER_SLOT].reshape(-1, 160)[:, FM].copy(),
            b"".join(sorted(x.tobytes() for x in recs)), c["simulations"])


def _z(status, player):
    return 0.0 if status == -2 else (1.0 if player == status else -1.0)


def retrace(P, sides, threads, kinds, base, shape):
    """the games of play(), one after the other.  sides: {P.PLAYER_ALPHAZERO: Side, P.PLAYER_ALPHAZERO_B: Side}; kinds: the kind of
    player 0 and of player 1.  [Game], slot by slot"""
    hs = {}
    for k in kinds:
        s = sides[k]
        h = engine(P, s, threads, 1, shape.rounds)
        if s.m > 0:
            h.set_gumbel(s.m, CV, CS)
            h.set_gumbel_tree(s.tree)
            h.set_root_gumbel(None)
            h.set_simulations(s.sims)
        hs[k] = h
    games = []
    for g, start in ((g, start) for g in range(shape.slots) for start in range(PER_SLOT)):
        first = hs[kinds[start]]
        first.new_games(np.array([base + g if start == 0 else int(rng[0])], np.uint32))
        state, rng = first.get_states(), first.get_rng()
        assert state[0][146] == 0
        state[0][146] = start
        rows, decisions, sims, in_turn = [], [], 0, False
        while True:
            p = int(state[0][146])
            h, s = hs[kinds[p]], sides[kinds[p]]
            h.set_states(state)
            h.set_rng(rng)
            n0 = 0
            if not in_turn:
                h.mcts_clear()
            elif s.m > 0:
                n0 = int(h.node_stats(state)[0][0].sum())
            valid = int(h.valid_moves()[0])
            h.simulate()
            if s.m > 0:
                pi, mv = h.gumbel_policy()[0][0], h.gumbel_pick()
            else:
                pi, mv = h.policy()[0], h.pick(sample=False)
            rec = np.zeros(265, np.uint8)
            rec[0] = p
            rec[1:89] = h.encode()[0]
            rec[93:265] = pi.view(np.uint8)
            rows.append(rec)
            decisions.append((n0, bin(valid & ((1 << 43) - 1)).count("1"), s.m))
            sims += s.sims - s.sims % threads
            assert (h.make_moves(mv) == 0).all()
            state, rng = h.get_states(), h.get_rng()
            status = int(h.status()[0])
            if status != -1:
                break
            in_turn = int(state[0][146]) == p
            assert len(rows) < 4000
        for rec in rows:
            rec[89:93] = np.array([_z(status, int(rec[0]))], f32).view(np.uint8)
        games.append(Game(start, np.array(rows, np.uint8), state[0].copy(), status, int(state[0][144]) + 256 * int(state[0][145]), sims, decisions))
    for h in hs.values():
        h.close()
    return games


def expected(games):
    """what play() returns for an arena that played `games`"""
    st = [x.status for x in games]
    won = lambda p, started: sum(x.status == p and (not started or x.start == p) for x in games)   # noqa: E731
    six = [len(games), st.count(-2), won(0, False), won(0, True), won(1, False), won(1, True)]
    recs = np.concatenate([x.records for x in games])
    return (six, st, [x.rounds for x in games], np.array([x.final[FM] for x in games]), b"".join(sorted(r.tobytes() for r in recs)),
            sum(x.simulations for x in games))


def assert_same(got, want):
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2], (got[:3], want[:3])
    assert (got[3] == want[3]).all()
    assert len(got[4]) == len(want[4]) and got[4] == want[4]
    assert got[5] == want[5], (got[5], want[5])
