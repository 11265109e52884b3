"""Resignation with a no-resign holdout, restated from include/azr.h in np.float32 and Python integers (TEST INFRASTRUCTURE): the
holdout coin, the per-game state update, the first decision at which a game gives up, and the holdout statistics of a set of games.
The root value q of a decision is value_mix_ref.root_value's.

tests/test_resign_ref.py checks the restatement on the CPU; tests/test_gpu_resign.py pins the device to it."""
import numpy as np

from playout_cap_ref import M32, mix

f32 = np.float32
NONE = 255


def threshold(holdout_share):
    """(uint32_t)(holdout_share * 16777216.0f), in float"""
    return int(f32(holdout_share) * f32(16777216.0))


def holdout(holdout_share, seed, game_seed):
    """True = the game with seed `game_seed` is held out"""
    k = mix(seed + 0x2545F491)
    k = mix(k ^ (game_seed & M32))
    k = mix((k + 0x68E31DA4) & M32)
    return (k >> 8) < threshold(holdout_share)


def holdout_many(holdout_share, seed, game_seeds):
    """the coin for every game seed, vectorised: bool [len(game_seeds)]"""
    def vmix(x):
        x = x.astype(np.uint64)
        x ^= x >> np.uint64(16); x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
        x ^= x >> np.uint64(15); x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
        x ^= x >> np.uint64(16)
        return x
    s = np.asarray(game_seeds, np.uint64) & np.uint64(M32)
    k = np.uint64(mix(seed + 0x2545F491))
    k = vmix(k ^ s)
    k = vmix((k + np.uint64(0x68E31DA4)) & np.uint64(M32))
    return (k >> np.uint64(8)) < np.uint64(threshold(holdout_share))


def step(run, p, q, has_q, q_resign, streak):
    """one decision of player p with the root value q: run (a list [run0, run1]) is updated in place; True = p gives up"""
    below = bool(has_q) and f32(q) < f32(q_resign)
    run[p] = min(run[p] + 1, 255) if below else 0
    return run[p] >= streak


def runs(q, has_q, player, q_resign, streak):
    """the state after every decision of one game that never stops: (run [n, 2], gives_up [n] bool)"""
    run, out, up = [0, 0], [], []
    for qq, hq, p in zip(q, has_q, player):
        up.append(step(run, int(p), qq, hq, q_resign, streak))
        out.append(list(run))
    return np.array(out, np.uint8).reshape(-1, 2), np.array(up, bool)


def first_resign(q, has_q, player, q_resign, streak):
    """(row, player) of the first decision of the game at which its mover gives up, (-1, 255) if nobody does"""
    run = [0, 0]
    for r, (qq, hq, p) in enumerate(zip(q, has_q, player)):
        if step(run, int(p), qq, hq, q_resign, streak):
            return r, int(p)
    return -1, NONE


def stats(games, q_resign, streak, holdout_share, seed):
    """games: per game (q, has_q, player, game seed, natural status: the winner, or -2 for a draw).  The four counts after all of them
    have ended, a resigning game at its resignation: dict as azr_selfplay_resign_stats reports"""
    s = dict(resigned=0, holdout_games=0, holdout_would_resign=0, holdout_not_lost=0)
    for q, has_q, player, game_seed, status in games:
        row, who = first_resign(q, has_q, player, q_resign, streak)
        if holdout(holdout_share, seed, game_seed):
            s["holdout_games"] += 1
            if row >= 0:
                s["holdout_would_resign"] += 1
                s["holdout_not_lost"] += int(status != 1 - who)
        elif row >= 0:
            s["resigned"] += 1
    return s
