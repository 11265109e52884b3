"""CPU: the composed AlphaZeroPlayer-vs-AlphaZeroPlayer driver (tests/arena_budget_ref.py: two orc_mcts objects, each with its own
orc_settings) reproduces the oracle's own game drivers — which are pinned to the reference — when both sides carry the SAME settings:
statuses, rounds, final states, every (s, pi, z) record and the six GameResults numbers, for the sequential mirrored form
(orc_play_games2) and the concurrent halves (orc_play_half_games), at one and two search threads.  Only then is the driver used with
different settings per side as the yardstick of the device arena (tests/test_gpu_arena_budget.py)."""
import ctypes as C

import numpy as np
import pytest

import arena_budget_ref as R
import azr_testlib as T


def _same(mine, theirs):
    r6, st, rd, fin, games, _ = mine
    o6, ost, ord_, ofin, ogames = theirs
    assert tuple(r6) == tuple(o6)
    assert (st == ost).all() and (rd == ord_).all()
    assert fin.tobytes() == ofin.tobytes()
    assert len(games) == len(ogames)
    for a, b in zip(games, ogames):
        assert len(a) > 0 and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("b_first", [False, True])
@pytest.mark.parametrize("threads", [1, 2])
def test_sequential_form_equals_orc_play_games2(orc, threads, b_first):
    k = (R.AZ_B, R.AZ_A) if b_first else (R.AZ_A, R.AZ_B)
    cfg = T.default_settings(mcts_simulations=9, mcts_threads=threads, max_game_rounds=40)
    ev = orc.orc_hash_eval
    for seed in (5200, 5201):
        want = T.orc_play_games2(k[0], k[1], 4, True, seed, cfg, ev, ev)
        got = R.play_games(k[0], k[1], 4, True, seed, cfg, cfg, ev, ev)
        _same(got, want)
        assert got[5] > 0 and got[5] % (9 - 9 % threads) == 0     # whole decisions of S - S % T simulations
    want = T.orc_play_games2(k[0], k[1], 3, False, 77, cfg, ev, ev)          # no mirroring: every game a fresh deal
    _same(R.play_games(k[0], k[1], 3, False, 77, cfg, cfg, ev, ev), want)


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("b_first", [False, True])
@pytest.mark.parametrize("threads", [1, 2])
def test_concurrent_halves_equal_orc_play_half_games(orc, threads, b_first, half):
    k = (R.AZ_B, R.AZ_A) if b_first else (R.AZ_A, R.AZ_B)
    cfg = T.default_settings(mcts_simulations=8, mcts_threads=threads, max_game_rounds=40)
    ev = orc.orc_hash_eval
    want = T.orc_play_half_games(k[0], k[1], 3, half, 9100, 3, cfg, ev, ev)
    _same(R.play_half_games(k[0], k[1], 3, half, 9100, 3, cfg, cfg, ev, ev), want)


def test_each_side_searches_with_its_own_settings(orc):
    """what the driver is for: with another budget on side B the games differ from the equal-settings ones, and the simulation count
    is what the two budgets give — every decision of a side costs that side's S - S % T"""
    ev = orc.orc_hash_eval
    a = T.default_settings(mcts_simulations=12, mcts_threads=2, max_game_rounds=40)
    b = T.default_settings(mcts_simulations=5, mcts_threads=2, max_game_rounds=40, hp_exploration=2.0)
    r6, st, rd, fin, games, sims = R.play_games(R.AZ_A, R.AZ_B, 2, True, 31, a, b, ev, ev)
    dec = [0, 0]
    for g in games:
        for rec in g:
            dec[int(rec[0])] += 1
    assert sims == 12 * dec[0] + 4 * dec[1] and dec[0] > 0 and dec[1] > 0      # player index 0 is side A in both games of the pair
    same = R.play_games(R.AZ_A, R.AZ_B, 2, True, 31, a, a, ev, ev)
    assert b"".join(g.tobytes() for g in games) != b"".join(g.tobytes() for g in same[4])
