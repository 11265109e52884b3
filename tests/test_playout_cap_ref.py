"""CPU: the composed self-play loop with a playout cap (tests/playout_cap_ref.py) against the oracle's own orc_selfplay_game — which
is pinned to the reference.  With full_prob = 1 it is orc_selfplay_game byte for byte, at one and two search threads; with the fast
budget equal to the full one the cap only gates the records, so the records are the rows of the uncapped stream whose coin is full;
and with two budgets the tree's simulation count is S * full + F * fast.  Only then is it the yardstick of the device's capped
self-play (tests/test_gpu_playout_cap.py)."""
import numpy as np
import pytest

import azr_testlib as T
import playout_cap_ref as R

SEEDS = range(4242, 4248)
CAP_SEED = 99


def _cfg(threads, sims=6):
    return T.default_settings(mcts_simulations=sims, max_game_rounds=36, mcts_threads=threads)


@pytest.mark.parametrize("threads", [1, 2])
def test_full_prob_one_is_orc_selfplay_game(orc, threads):
    cfg = _cfg(threads)
    for seed in SEEDS:
        want, st, sims = R.oracle_game(cfg, seed, orc.orc_hash_eval)
        for prob, fast in ((1.0, 2), (0.5, 0)):          # both spellings of "off"
            got, kinds, gst, gsims = R.selfplay_game(cfg, seed, orc.orc_hash_eval, prob, fast, CAP_SEED)
            assert got.tobytes() == want.tobytes() and gst == st and gsims == sims
            assert kinds.all() and len(kinds) == len(want)


@pytest.mark.parametrize("threads", [1, 2])
def test_equal_budgets_only_gate_the_records(orc, threads):
    cfg = _cfg(threads)
    for seed in SEEDS:
        want, st, sims = R.oracle_game(cfg, seed, orc.orc_hash_eval)
        got, kinds, gst, gsims = R.selfplay_game(cfg, seed, orc.orc_hash_eval, 0.5, 6, CAP_SEED)
        assert len(kinds) == len(want) and gst == st and gsims == sims
        coin = np.array([R.coin(0.5, CAP_SEED, seed, d) for d in range(len(want))])
        assert (kinds == coin).all() and 0 < coin.sum() < len(coin)
        assert got.tobytes() == want[coin].tobytes()


@pytest.mark.parametrize("threads", [1, 2])
def test_simulations_are_the_two_budgets(orc, threads):
    cfg = _cfg(threads)
    for seed in SEEDS:
        got, kinds, gst, sims = R.selfplay_game(cfg, seed, orc.orc_hash_eval, 0.5, 2, CAP_SEED)
        full, fast = int(kinds.sum()), int((kinds == 0).sum())
        assert full >= 10 and fast >= 10 and len(got) == full
        assert sims == 6 * full + 2 * fast


def test_the_coin_restatements_agree():
    """the scalar and the vectorised restatement of the header's formula; P = 0 and P = 1; another cap seed, another pattern"""
    s, d = np.arange(1000, 1016), np.arange(0, 64)
    g = R.coin_grid(0.25, CAP_SEED, s, d)
    assert all(bool(g[i, j]) == R.coin(0.25, CAP_SEED, int(s[i]), int(d[j])) for i in range(len(s)) for j in range(len(d)))
    assert not R.coin_grid(0.0, CAP_SEED, s, d).any() and R.coin_grid(1.0, CAP_SEED, s, d).all()
    assert (g != R.coin_grid(0.25, CAP_SEED + 1, s, d)).any()
    assert R.threshold(0.25) == 1 << 22 and R.threshold(0.0) == 0
