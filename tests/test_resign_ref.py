"""CPU: tests/resign_ref.py, the restatement of include/azr.h's resignation rule that tests/test_gpu_resign.py pins the device to.  The
holdout coin's share and its independence of the playout cap's and the copy coin's at equal seeds; the state update on hand-written
series."""
import math

import numpy as np
import pytest

import playout_cap_ref as R
import resign_ref as RS
import surprise_ref as S

f32 = np.float32


# ---- the coin ---------------------------------------------------------------------------------------------------------------------
N_SEEDS = 100_000


def _within(count, n, p, sigmas=5.0):
    """a binomial(n, p) count lies within 5 standard deviations of n p with probability above 1 - 6e-7; the coin is a fixed function, so
    the check either always passes or always fails — the bound says what a hash that behaves like a fair coin may do"""
    return abs(count - n * p) <= sigmas * math.sqrt(n * p * (1.0 - p))


@pytest.mark.parametrize("seed", [0, 7, 0xFFFFFFFF])
@pytest.mark.parametrize("share", [0.1, 0.5, 0.9])
def test_the_coin_holds_out_its_share(share, seed):
    seeds = np.arange(20260001, 20260001 + N_SEEDS, dtype=np.uint64)
    held = RS.holdout_many(share, seed, seeds)
    p = RS.threshold(share) / 16777216.0
    assert abs(p - share) < 2.0 ** -24 * 2
    assert _within(int(held.sum()), N_SEEDS, p), (share, seed, int(held.sum()))


def test_share_zero_holds_nothing_out_and_share_one_everything():
    seeds = np.arange(0, 5000, dtype=np.uint64)
    assert not RS.holdout_many(0.0, 3, seeds).any()
    assert RS.holdout_many(1.0, 3, seeds).all()
    assert RS.threshold(1.0) == 1 << 24 and RS.threshold(0.0) == 0


def test_the_vectorised_coin_is_the_scalar_one():
    seeds = [0, 1, 599, 600, 20260001, 0xFFFFFFFF, 0x80000000]
    for share in (0.1, 0.5):
        for seed in (0, 9, 0xFFFFFFFF):
            assert RS.holdout_many(share, seed, seeds).tolist() == [RS.holdout(share, seed, s) for s in seeds]


def test_the_coin_depends_on_seed_and_game_seed():
    seeds = np.arange(1000, 3000, dtype=np.uint64)
    a, b = RS.holdout_many(0.5, 1, seeds), RS.holdout_many(0.5, 2, seeds)
    assert a.any() and not a.all() and (a != b).any()


@pytest.mark.parametrize("seed", [0, 31])
def test_the_coin_is_not_the_caps_nor_the_copy_coin_at_equal_seeds(seed):
    """at share 1/2 and equal seeds, the holdout coin and another fair coin agree on a game with probability 1/2 if they are
    independent: the count of agreements over n games is binomial(n, 1/2), bound as above.  Against the playout cap's coin of decision 0
    (and 1), and the copy coin of record 0 at weight 1/2."""
    n = N_SEEDS
    seeds = np.arange(600, 600 + n, dtype=np.uint64)
    held = RS.holdout_many(0.5, seed, seeds)
    for d in (0, 1):
        cap = R.coin_grid(0.5, seed, seeds, [d])[:, 0].astype(bool)
        assert _within(int((held == cap).sum()), n, 0.5), (d, int((held == cap).sum()))
    m = 20_000
    copy = np.array([S.copies(0.5, seed, int(s), 0) for s in seeds[:m]], bool)
    assert _within(int(copy.sum()), m, 0.5)
    assert _within(int((held[:m] == copy).sum()), m, 0.5), int((held[:m] == copy).sum())


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
QR = f32(-0.5)
LOW, OK = f32(-0.75), f32(0.25)


def _game(series):
    """series of (player, q, has_q) -> the three columns"""
    return [s[1] for s in series], [s[2] for s in series], [s[0] for s in series]


def test_a_streak_broken_by_one_good_value_starts_over():
    q, has, pl = _game([(0, LOW, 1), (0, LOW, 1), (0, OK, 1), (0, LOW, 1), (0, LOW, 1), (0, LOW, 1)])
    run, up = RS.runs(q, has, pl, QR, 3)
    assert run[:, 0].tolist() == [1, 2, 0, 1, 2, 3] and not run[:, 1].any()
    assert up.tolist() == [False] * 5 + [True]
    assert RS.first_resign(q, has, pl, QR, 3) == (5, 0)
    assert RS.first_resign(q[:5], has[:5], pl[:5], QR, 3) == (-1, RS.NONE)


def test_the_other_players_decisions_in_between_do_not_break_a_streak():
    q, has, pl = _game([(1, LOW, 1), (0, OK, 1), (0, OK, 1), (1, LOW, 1), (0, OK, 1), (1, LOW, 1)])
    run, up = RS.runs(q, has, pl, QR, 3)
    assert run[:, 1].tolist() == [1, 1, 1, 2, 2, 3] and not run[:, 0].any()
    assert RS.first_resign(q, has, pl, QR, 3) == (5, 1)
    # ... and each player has a run of its own: 0 is low too, one decision later, and 1 is there first
    q, has, pl = _game([(1, LOW, 1), (0, LOW, 1), (1, LOW, 1), (0, LOW, 1)])
    assert RS.first_resign(q, has, pl, QR, 2) == (2, 1)


def test_a_decision_without_a_root_value_resets_the_run():
    q, has, pl = _game([(0, LOW, 1), (0, LOW, 0), (0, LOW, 1), (0, LOW, 1)])
    run, up = RS.runs(q, has, pl, QR, 2)
    assert run[:, 0].tolist() == [1, 0, 1, 2] and up.tolist() == [False, False, False, True]


def test_a_run_saturates_at_255():
    n = 300
    run, up = RS.runs([LOW] * n, [1] * n, [0] * n, QR, 255)
    assert run[:, 0].tolist() == list(range(1, 256)) + [255] * (n - 255)
    assert up.tolist() == [False] * 254 + [True] * (n - 254)
    run, up = RS.runs([LOW] * n + [OK], [1] * (n + 1), [0] * (n + 1), QR, 255)
    assert run[-1, 0] == 0 and not up[-1]


def test_a_value_at_the_bound_is_not_below_it():
    below = np.nextafter(QR, f32(-2), dtype=f32)
    above = np.nextafter(QR, f32(2), dtype=f32)
    assert RS.first_resign([QR], [1], [0], QR, 1) == (-1, RS.NONE)
    assert RS.first_resign([above], [1], [0], QR, 1) == (-1, RS.NONE)
    assert RS.first_resign([below], [1], [1], QR, 1) == (0, 1)
    # the bound may be positive
    assert RS.first_resign([f32(0.25)], [1], [0], f32(0.5), 1) == (0, 0)


def test_streak_one_gives_up_at_the_first_low_value():
    q, has, pl = _game([(0, OK, 1), (1, OK, 1), (0, LOW, 1), (1, LOW, 1)])
    assert RS.first_resign(q, has, pl, QR, 1) == (2, 0)


def test_statistics_of_a_set_of_games():
    low3 = ([LOW] * 3, [1] * 3, [0, 1, 0])                       # player 0 gives up at row 0 under streak 1
    fine = ([OK] * 3, [1] * 3, [0, 1, 0])
    seeds = [s for s in range(600, 700)]
    held = [s for s in seeds if RS.holdout(0.5, 5, s)]
    free = [s for s in seeds if not RS.holdout(0.5, 5, s)]
    assert len(held) >= 3 and len(free) >= 2
    games = [low3 + (held[0], 1), low3 + (held[1], 0), low3 + (held[2], -2), fine + (held[3], 0), low3 + (free[0], 0), fine + (free[1], 1)]
    assert RS.stats(games, QR, 1, 0.5, 5) == dict(resigned=1, holdout_games=4, holdout_would_resign=3, holdout_not_lost=2)
    assert RS.stats(games, QR, 1, 1.0, 5) == dict(resigned=0, holdout_games=6, holdout_would_resign=4, holdout_not_lost=3)
    assert RS.stats(games, QR, 1, 0.0, 5) == dict(resigned=4, holdout_games=0, holdout_would_resign=0, holdout_not_lost=0)
