"""AlphaZeroPlayer against AlphaZeroPlayer, each with an AlphaZeroMCTS and Settings of its own (TEST INFRASTRUCTURE).

The oracle's game drivers (orc_play_games2, orc_play_half_games) give both players one orc_settings.  This module composes the same
games in Python from the oracle's exported pieces — two orc_mcts objects, each created from its own orc_settings, orc_new_game,
orc_mcts_simulate, orc_mcts_policy, orc_pick_highest, orc_make_move, orc_invert_players, orc_update_values — so that the two players
may differ in mcts_simulations and hp_exploration:

  Game::playTurn / gameLoop             game.cpp:112-133   -> play_out
  Game::newGame, mirrored pairs         game.cpp:170-191   -> play_games (one slot of the sequential form)
  the concurrent halves of a pair       include/azr.h, AZR_MIRROR_CONCURRENT -> play_half_games
  AlphaZeroPlayer::takeTurn             alphazero_player.cpp:3-21 -> az_take_turn

tests/test_arena_budget_ref.py pins it to the oracle's own drivers with equal settings on both sides."""
import ctypes as C

import numpy as np

import azr_testlib as T

AZ_A, AZ_B = 0, 3          # AZR_PLAYER_ALPHAZERO, AZR_PLAYER_ALPHAZERO_B
NOT_ENDED, DRAW, SETUP = -1, -2, 0


class Side:
    """one AlphaZeroPlayer: its search settings, its evaluator and its tree (kept over the slot's games, cleared at every newGame)"""

    def __init__(self, cfg, eval_fn):
        self.cfg, self.eval = cfg, eval_fn
        self.m = T.oracle().orc_mcts_create(C.byref(cfg))

    def close(self):
        T.oracle().orc_mcts_destroy(self.m)
        self.m = None


class Table:
    def __init__(self, kind0, kind1, cfg_a, cfg_b, eval_a, eval_b):
        assert {kind0, kind1} == {AZ_A, AZ_B}, "two AlphaZero players, one of each kind"
        sides = {AZ_A: Side(cfg_a, eval_a), AZ_B: Side(cfg_b, eval_b)}
        self.player = [sides[kind0], sides[kind1]]
        self.rules = cfg_a            # the rules of the game are one set (azr_settings of the arena handle)
        self.rec = []                 # 265-byte records of the running game
        self.games = []               # per finished game: its records, z filled in
        self.res = [0] * 6
        self.status, self.rounds, self.finals = [], [], []

    def sims(self):
        L = T.oracle()
        return sum(int(L.orc_mcts_sim_count(p.m)) for p in self.player)

    def close(self):
        for p in self.player:
            p.close()


def az_take_turn(side, s, me, r, rules, rec):
    """AlphaZeroPlayer::takeTurn (alphazero_player.cpp:3-21): trim, then search / argmax / move while it is this player's turn"""
    L = T.oracle()
    L.orc_mcts_trim(side.m)
    while L.orc_game_status(C.byref(s), C.byref(rules)) == NOT_ENDED and s.cur == me:
        rc = L.orc_mcts_simulate(side.m, C.byref(s), C.byref(r), side.eval, None)
        if rc:
            return rc
        pi = np.zeros(43, np.float32)
        rc = L.orc_mcts_policy(side.m, C.byref(s), T.ptr(pi))
        if rc:
            return rc
        li = L.orc_pick_highest(T.ptr(pi))
        d = np.zeros(265, np.uint8)     # addTrainingSample (alphazero_player.cpp:15-18): player | in88 | z (later) | pi
        d[0] = s.cur
        L.orc_encode(C.byref(s), T.ptr(d[1:89]))
        d[93:265] = pi.view(np.uint8)
        rec.append(d)
        rc = L.orc_make_move(C.byref(s), li, C.byref(r), C.byref(rules))
        if rc:
            return rc
    return 0


def play_out(t, s, r, player_start):
    """Game::gameLoop and the bookkeeping behind it (game.cpp:101-168) for one game that starts in state s"""
    L = T.oracle()
    for p in t.player:
        L.orc_mcts_clear(p.m)         # AlphaZeroPlayer::newGame
    gs = NOT_ENDED
    while gs == NOT_ENDED:            # Game::playTurn (game.cpp:112-133)
        cur, setup = s.cur, s.phase == SETUP
        rc = az_take_turn(t.player[cur], s, cur, r, t.rules, t.rec)
        assert rc == 0, rc
        gs = NOT_ENDED if setup else L.orc_game_status(C.byref(s), C.byref(t.rules))
        assert not (cur == s.cur and gs == NOT_ENDED), "Turn was not incremented"
    n = len(t.rec)
    players = np.array([d[0] for d in t.rec], np.int8)
    z = np.zeros(max(n, 1), np.float32)
    L.orc_update_values(T.ptr(players), n, gs, T.ptr(z))   # NNTrainDataStorage::updateValues for both players
    for d, zi in zip(t.rec, z):
        d[89:93] = np.array([zi], np.float32).view(np.uint8)
    t.games.append(np.array(t.rec, np.uint8).reshape(n, 265))
    t.rec = []
    t.res[0] += 1                     # GameResults::addGame (game.cpp:193-213)
    if gs == DRAW:
        t.res[1] += 1
    for p in range(2):
        if gs == p:
            t.res[2 + 2 * p] += 1
            if player_start == p:
                t.res[3 + 2 * p] += 1
    fin = np.zeros(160, np.uint8)
    L.orc_state_pack(C.byref(s), T.ptr(fin))
    t.status.append(gs); t.rounds.append(s.round); t.finals.append(fin)


def _result(t):
    out = (tuple(t.res), np.array(t.status, np.int8), np.array(t.rounds, np.uint16), np.array(t.finals, np.uint8).reshape(-1, 160),
           t.games, t.sims())
    t.close()
    return out


def _copy_state(s):
    c = T.OrcState()
    C.memmove(C.byref(c), C.byref(s), C.sizeof(T.OrcState))
    return c


def play_games(kind0, kind1, games, mirror, seed, cfg_a, cfg_b, eval_a, eval_b):
    """one slot of the sequential form (orc_play_games2): `games` games with alternating starts, mirrored pairs (Game::newGame,
    game.cpp:170-191), one RNG stream for everything.  Returns (six results, status, rounds, finals, records per game, simulations)"""
    L = T.oracle()
    t = Table(kind0, kind1, cfg_a, cfg_b, eval_a, eval_b)
    r = T.OrcRng()
    L.orc_rng_seed(C.byref(r), seed)
    s, prev_start = T.OrcState(), None
    player_start = 0
    for _ in range(games):
        if mirror and player_start != 0:
            s = _copy_state(prev_start)
            L.orc_invert_players(C.byref(s))
            s.cur = player_start
        else:
            L.orc_new_game(C.byref(s), C.byref(r))
            s.cur = player_start
            prev_start = _copy_state(s)
        play_out(t, s, r, player_start)
        player_start = (player_start + 1) % 2
    return _result(t)


def play_half_games(kind0, kind1, games, half, pair_seed0, pair_stride, cfg_a, cfg_b, eval_a, eval_b):
    """one slot of the concurrent halves (orc_play_half_games; the rule is in include/azr.h): half `half` of the pairs pair_seed0 +
    k * pair_stride — both halves deal from minstd_rand0(q); half 1 inverts the deal, starts with player 1 and draws its dice from
    minstd_rand0(q + 2^30)"""
    L = T.oracle()
    t = Table(kind0, kind1, cfg_a, cfg_b, eval_a, eval_b)
    r = T.OrcRng()
    for gi in range(games):
        q = (pair_seed0 + gi * pair_stride) & 0xffffffff
        s = T.OrcState()
        L.orc_rng_seed(C.byref(r), q)
        L.orc_new_game(C.byref(s), C.byref(r))
        if half:
            L.orc_invert_players(C.byref(s))
            L.orc_rng_seed(C.byref(r), (q + (1 << 30)) & 0xffffffff)
        s.cur = half
        play_out(t, s, r, half)
    return _result(t)
