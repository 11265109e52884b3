"""GPU: resignation with a no-resign holdout in device self-play (azr_selfplay_set_resign, azr_selfplay_resign_stats,
azr_selfplay_resign_state, azr_debug_resign).  The contract is include/azr.h's; tests/resign_ref.py restates it.  Checked here: the rule
alone on the device against the restatement, bit for bit; a resigned game is a prefix of the game without resignation — the late golden
games of tests/selfplay_retrace.py retraced decision by decision through the host-stepped entry points give every game's rows, the
restatement cuts them, and the device's stream must hold exactly the cut games with z rewritten for the resignation (one and two search
threads, streak 1 and 2, under the value mix, under surprise weighting, under a playout cap); the holdout and its statistics; slot
independence; the setter's contract.
Engines of 8 games, one block, NET_F32, 8 simulations."""
import numpy as np
import pytest

import resign_ref as RS
import selfplay_retrace as SR
import surprise_ref as S
import value_mix_ref as V
from gpu_common import pi_of, pkg

pytestmark = pytest.mark.gpu
f32 = np.float32
G = 8
BASE, CSEED, SIMS, FAST, QUOTA = 9100, 99, 8, 4, 4      # the games of test_gpu_value_mix: one retrace serves both files
SHARE, MAXW, PSEED = 0.75, 4.0, 31                      # surprise weighting
QSHARE = 0.5                                            # value mix
RSEED = 5                                               # the holdout coin's seed where nothing is held out


# ---- 1. the rule alone, bit for bit ---------------------------------------------------------------------------------------------------
def _synthetic_games(q_resign):
    """64 games of 1..40 decisions, both players to move in runs of random length; q at, one ulp below and one ulp above q_resign, far
    below and far above it, has_q mostly set; the first games are hand-made"""
    rng = np.random.default_rng(41)
    qr = f32(q_resign)
    below, above = np.nextafter(qr, f32(-2), dtype=f32), np.nextafter(qr, f32(2), dtype=f32)
    pool = np.array([qr, below, above, f32(-1.0), f32(1.0), qr - f32(0.25), qr + f32(0.25)], f32)
    games = [([below], [1], [0]), ([qr], [1], [1]), ([above], [1], [0]), ([below] * 5, [1] * 5, [1] * 5),
             ([below] * 5, [1, 1, 0, 1, 1], [0] * 5), ([below, below, qr, below, below, below, below, below], [1] * 8, [0] * 8),
             ([below] * 9, [1] * 9, [0, 1, 0, 1, 0, 1, 0, 1, 0])]
    while len(games) < 64:
        n = 40 if len(games) == 7 else int(rng.integers(1, 41))
        pl, p = [], int(rng.integers(0, 2))
        while len(pl) < n:
            pl += [p] * int(rng.integers(1, 7))
            p = 1 - p
        q = pool[rng.choice(len(pool), n, p=[0.1, 0.35, 0.1, 0.15, 0.05, 0.15, 0.1])]
        games.append((q, (rng.random(n) < 0.92).astype(np.uint8), pl[:n]))
    lens = np.array([len(g[0]) for g in games], np.uint32)
    assert lens.min() == 1 and lens.max() == 40 and len(games) == 64
    seeds = (np.arange(64, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(600))
    return games, lens, seeds


@pytest.mark.parametrize("holdout_share", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("streak", [1, 2, 5])
def test_the_rule_on_the_device_is_the_restatement(streak, holdout_share):
    q_resign = -0.3
    games, lens, seeds = _synthetic_games(q_resign)
    want = [RS.first_resign(q, has, pl, q_resign, streak) for q, has, pl in games]
    held = RS.holdout_many(holdout_share, 17, seeds)
    # conditions of the cases, on the restatement: both players give up somewhere, some game never does, and the coin splits the games
    assert {w[1] for w in want} == {0, 1, RS.NONE}, streak
    assert want[1] == (-1, RS.NONE) and want[2] == (-1, RS.NONE) and (want[0] == (0, 0)) == (streak == 1)
    assert held.all() if holdout_share == 1.0 else not held.any() if holdout_share == 0.0 else (held.any() and not held.all())
    P = pkg()
    eng = P.Engine(2, blocks=1, sims=SIMS, dtype=P.NET_F32)
    row, who, hold = eng.debug_resign(q_resign, streak, holdout_share, 17, np.concatenate([np.asarray(g[0], f32) for g in games]),
                                      np.concatenate([np.asarray(g[1], np.uint8) for g in games]),
                                      np.concatenate([np.asarray(g[2], np.uint8) for g in games]), lens, seeds)
    eng.close()
    assert row.tolist() == [w[0] for w in want], (row, want)
    assert who.tolist() == [w[1] for w in want]
    assert hold.tolist() == held.tolist()


def test_a_run_saturates_on_the_device():
    P = pkg()
    eng = P.Engine(2, blocks=1, sims=SIMS, dtype=P.NET_F32)
    n = 300
    q, has, pl = np.full(n, -0.5, f32), np.ones(n, np.uint8), np.zeros(n, np.uint8)
    row, who, _ = eng.debug_resign(0.0, 255, 0.0, 0, q, has, pl, [n], [1])
    assert (int(row[0]), int(who[0])) == RS.first_resign(q, has, pl, 0.0, 255) == (254, 0)
    has[200] = 0                                                     # a decision without a value: the run starts over, 99 are left
    row, who, _ = eng.debug_resign(0.0, 255, 0.0, 0, q, has, pl, [n], [1])
    assert (int(row[0]), int(who[0])) == RS.first_resign(q, has, pl, 0.0, 255) == (-1, RS.NONE)
    eng.close()


# ---- 2. a resigned game is a prefix of the game without resignation ----------------------------------------------------------------
def _run(threads, cap=False, psw=False, mix=False, net="base"):
    return SR.Run(BASE, QUOTA, threads, SIMS, surprise=(SHARE, MAXW, PSEED) if psw else None, value_mix=QSHARE if mix else None, net=net,
                  **(dict(fast=FAST, cap=(0.5, CSEED)) if cap else {}))


def _series(game):
    """(q [n] float32, has_q [n] bool, player [n]) of a retraced game's recorded decisions, q by value_mix_ref from N, Q and valid"""
    qh = [V.root_value(n, qq, va) for n, qq, va in zip(game.N, game.Q, game.valid)]
    return np.array([x[0] for x in qh], f32), np.array([x[1] for x in qh], bool), game.records[:, 0].astype(int)


def _status(game):
    """the natural end of a retraced game from its records' z: the winner, or -2 for a draw"""
    if not game.z.any():
        return -2
    r = int(np.flatnonzero(game.z)[0])
    p = int(game.records[r, 0])
    return p if game.z[r] > 0 else 1 - p


def _cuts(series, q_resign, streak):
    return [RS.first_resign(q, has, pl, q_resign, streak) for q, has, pl in series]


def _q_resign(series, streak):
    """A bound derived from the retraced q series: the midpoints between adjacent distinct values of q for which the restatement lets
    at least one game resign strictly before its last recorded decision and at least one game reach its end; of those the one under
    which the most games resign early, the lowest on ties.  One run gives both outcomes: such a value must exist."""
    allq = np.unique(np.concatenate([s[0] for s in series]))
    best = None
    for a, b in zip(allq[:-1], allq[1:]):
        mid = f32((a + b) * f32(0.5))
        if not a < mid < b:
            continue
        cuts = _cuts(series, mid, streak)
        early = sum(1 for (row, _), s in zip(cuts, series) if 0 <= row < len(s[0]) - 1)
        if early and any(row < 0 for row, _ in cuts) and (best is None or early > best[0]):
            best = (early, mid)
    assert best is not None, "no midpoint of the retraced q series lets one game resign early and another reach its end"
    return float(best[1])


def _expected(game, series, cut, who, psw, mix, seed):
    """(records, copies or None) the device writes for a game: all of it as retraced when it does not resign (cut < 0), else its rows up
    to and including the cut with z for the status 1 - who; under the value mix z' by value_mix_ref, under surprise weighting the copy
    counts by surprise_ref from the rows that are left"""
    q, has, pl = series
    n = len(q) if cut < 0 else cut + 1
    status = _status(game) if cut < 0 else 1 - who
    recs = game.records[:n].copy()
    for r in range(n):
        z = f32(SR.outcome_z(status, int(pl[r])))
        if mix:
            z = V.blend(z, q[r], has[r], QSHARE)
        recs[r, 89:93] = np.array([z], f32).view(np.uint8)
    copies = None
    if psw:
        kl = np.array([S.record_kl(pi, pr, va) for pi, pr, va in zip(pi_of(recs), game.prior[:n], game.valid[:n])], f32)
        copies = S.game_copies(kl, SHARE, MAXW, PSEED, seed)[1]
    return recs, copies


def assert_exactly_these_streams(records, streams):
    """every game's expected records lie side by side, record-aligned, in the device's bytes, each game in bytes of its own, and the
    device wrote nothing else"""
    blob = records.tobytes()
    for g, (want, copies) in enumerate(streams):
        stream = (want if copies is None else np.repeat(want, copies, axis=0)).tobytes()
        assert len(want) > 0
        at = blob.find(stream)
        while at >= 0 and at % 265:
            at = blob.find(stream, at + 1)
        assert at >= 0, f"game {g}: its record stream is not in the device's output"
        blob = blob[:at] + blob[at + len(stream):]
    assert len(blob) == 0, f"{len(blob) // 265} records of the device belong to no game"


def _play(run, q_resign, streak, holdout_share=0.0, seed=RSEED, after_run=None):
    eng = SR.selfplay(run, lambda e: e.selfplay_set_resign(q_resign, streak, holdout_share, seed))
    if after_run:
        after_run(-1, eng)
    recs, c = SR.play_out(eng, run.quota, 16, 400, after_run=after_run)
    stats = eng.selfplay_resign_stats()
    eng.close()
    return recs, c, stats


@pytest.mark.parametrize("threads,streak,cap,psw,mix", [(1, 1, False, False, False), (1, 2, False, False, False), (2, 1, False, False, False),
                                                       (2, 2, False, False, False), (2, 2, False, False, True), (2, 1, False, True, False),
                                                       (2, 2, True, False, False)])
def test_a_resigned_game_is_a_prefix_of_the_retraced_game(threads, streak, cap, psw, mix):
    run = _run(threads, cap, psw, mix)
    games, tot = SR.cached("retrace", run)
    series = [_series(g) for g in games]
    q_resign = _q_resign(series, streak)
    cuts = _cuts(series, q_resign, streak)
    print("q_resign %.6f, streak %d: cut rows %s of %s rows, resigners %s" %
          (q_resign, streak, [c[0] for c in cuts], [len(s[0]) for s in series], [c[1] for c in cuts]))
    recs, c, stats = _play(run, q_resign, streak)
    streams = [_expected(game, s, row, who, psw, mix, BASE + g) for g, (game, s, (row, who)) in enumerate(zip(games, series, cuts))]
    assert_exactly_these_streams(recs, streams)
    total = sum(len(w) if k is None else int(k.sum()) for w, k in streams)
    resigned = sum(1 for row, _ in cuts if row >= 0)
    assert len(recs) == total == c["samples"] and c["games_finished"] == QUOTA and c["errors"] == 0
    assert stats == dict(resigned=resigned, holdout_games=0, holdout_would_resign=0, holdout_not_lost=0), stats
    if not cap:   # (under a cap the rows are the full decisions only: the fast ones in between are counted too)
        decisions = sum(len(s[0]) if row < 0 else row + 1 for s, (row, _) in zip(series, cuts))
        assert decisions < tot["decisions"]
        assert c["decisions"] == decisions and c["simulations"] == decisions * (SIMS - SIMS % threads), (c, decisions)
    else:
        assert c["decisions"] < tot["decisions"] and c["simulations"] < tot["simulations"]


@pytest.mark.parametrize("threads", [1, 2])
def test_sharp_net_resigns_on_saturated_values(threads):
    """the same comparison on the sharp net (selfplay_retrace's Run.net), streak 1 and q_resign = -0.9: the root values that trigger it
    are means of Q = -1 exactly, and a resigned game is still the prefix of the retraced one"""
    run = _run(threads, net="sharp")
    games, tot = SR.cached("retrace", run)
    series = [_series(g) for g in games]
    q_resign, streak = -0.9, 1
    cuts = _cuts(series, q_resign, streak)
    allq = np.concatenate([s[0] for s in series])
    print("cut rows %s of %s rows, resigners %s; root values of exactly -1: %d, of exactly +1: %d" %
          ([c[0] for c in cuts], [len(s[0]) for s in series], [c[1] for c in cuts], (allq == -1).sum(), (allq == 1).sum()))
    resigned = sum(1 for row, _ in cuts if row >= 0)
    assert resigned > 0 and (allq <= f32(q_resign)).any()                  # the condition of the case, on the retrace: somebody gives up
    recs, c, stats = _play(run, q_resign, streak)
    streams = [_expected(game, s, row, who, False, False, BASE + g) for g, (game, s, (row, who)) in enumerate(zip(games, series, cuts))]
    assert_exactly_these_streams(recs, streams)
    decisions = sum(len(s[0]) if row < 0 else row + 1 for s, (row, _) in zip(series, cuts))
    assert len(recs) == sum(len(w) for w, _ in streams) == c["samples"] and c["games_finished"] == QUOTA
    assert c["errors"] == 0 and c["nodes_dropped"] == 0 and c["records_dropped"] == 0
    assert c["decisions"] == decisions and c["simulations"] == decisions * (SIMS - SIMS % threads), (c, decisions)
    assert stats == dict(resigned=resigned, holdout_games=0, holdout_would_resign=0, holdout_not_lost=0), stats


# ---- 3. the holdout ---------------------------------------------------------------------------------------------------------------
def _ref_games(games, series):
    return [(q, has, pl, BASE + g, _status(game)) for g, (game, (q, has, pl)) in enumerate(zip(games, series))]


def test_a_held_out_run_is_the_run_without_the_feature_and_counts_what_it_would_have_done():
    run = _run(2)
    games, _ = SR.cached("retrace", run)
    series = [_series(g) for g in games]
    q_resign = _q_resign(series, 1)
    never, c0 = SR.cached("selfplay", run)
    recs, c, stats = _play(run, q_resign, 1, holdout_share=1.0)
    assert recs.tobytes() == never.tobytes() and c == c0
    want = RS.stats(_ref_games(games, series), q_resign, 1, 1.0, RSEED)
    print(stats)
    assert stats == want and stats["resigned"] == 0 and stats["holdout_games"] == QUOTA and 0 < stats["holdout_would_resign"] < QUOTA


def _states(series, q_resign, streak):
    """every (run0, run1, first) a held-out game passes through, the start included"""
    q, has, pl = series
    run, first, seen = [0, 0], RS.NONE, {(0, 0, RS.NONE)}
    for qq, hq, p in zip(q, has, pl):
        if RS.step(run, int(p), qq, hq, q_resign, streak) and first == RS.NONE:
            first = int(p)
        seen.add((run[0], run[1], first))
    return seen


def test_the_coin_splits_held_out_and_resigning_games():
    streak = 2
    run = _run(2)
    games, _ = SR.cached("retrace", run)
    series = [_series(g) for g in games]
    q_resign = _q_resign(series, streak)
    cuts = _cuts(series, q_resign, streak)
    would = [g for g, (row, _) in enumerate(cuts) if row >= 0]
    # a seed of the coin under which one would-be resigner is held out and another is not (searched on the restatement)
    seed = next((s for s in range(256) if len({RS.holdout(0.5, s, BASE + g) for g in would}) == 2), None)
    assert len(would) >= 2 and seed is not None, (cuts, seed)
    held = [RS.holdout(0.5, seed, BASE + g) for g in range(QUOTA)]
    seen = []

    def look(i, eng):
        """before the first decision is over, and after every run of passes: the coin of the running games, and a state each held-out
        game passes through by the restatement"""
        fin = eng.counters()["games_finished"]
        run_, first, hold = eng.selfplay_resign_state()
        seen.append((i, fin, run_.tolist(), first.tolist(), hold.tolist()))
        assert not hold[QUOTA:].any() and not run_[QUOTA:].any() and (first[QUOTA:] == RS.NONE).all()      # idle slots
        if fin == 0:
            assert hold[:QUOTA].tolist() == held, (i, hold, held)
        for g in range(QUOTA):
            if hold[g]:
                assert held[g] and (int(run_[g, 0]), int(run_[g, 1]), int(first[g])) in _states(series[g], q_resign, streak), (i, g)

    def before(i, eng):
        if i == -1:
            eng.selfplay_run(3)        # (a decision takes S / T = 4 passes and more: nothing is decided yet)
            assert eng.counters()["decisions"] == 0
        look(i, eng)

    recs, c, stats = _play(run, q_resign, streak, holdout_share=0.5, seed=seed, after_run=before)
    assert seen[0][1] == 0 and any(any(f != RS.NONE for f in s[3]) for s in seen), seen
    streams = [_expected(game, s, -1 if held[g] else row, who, False, False, BASE + g)
               for g, (game, s, (row, who)) in enumerate(zip(games, series, cuts))]
    assert_exactly_these_streams(recs, streams)
    want = RS.stats(_ref_games(games, series), q_resign, streak, 0.5, seed)
    print(stats, "held out:", held, "cuts:", cuts)
    assert stats == want and stats["resigned"] >= 1 and stats["holdout_would_resign"] >= 1
    assert c["games_finished"] == QUOTA and c["samples"] == len(recs)


# ---- 4. independence of the layout ------------------------------------------------------------------------------------------------
def test_a_quota_resigns_the_same_games_on_four_eight_and_sixteen_slots():
    # the bound: the median root value of the same fresh games' records, read from a run under the value mix at share 1 (z' = q)
    probe = SR.quota_on_slots((8,), lambda eng: eng.selfplay_set_value_mix(1.0), SIMS, BASE)
    q = probe[0][:, 89:93].copy().view(f32)[:, 0]
    q_resign = float(np.median(q))
    stats = []

    def configure(eng):
        eng.selfplay_set_resign(q_resign, 2, 0.5, 3)
        close = eng.close

        def close_and_keep():
            stats.append(eng.selfplay_resign_stats())
            close()
        eng.close = close_and_keep

    recs, decisions, simulations, samples = SR.quota_on_slots((4, 8, 16), configure, SIMS, BASE)
    print("q_resign %.6f: %d records against %d, %s" % (q_resign, samples, probe[3], stats[0]))
    assert len(stats) == 3 and stats[0] == stats[1] == stats[2]
    assert stats[0]["resigned"] >= 1 and stats[0]["holdout_games"] >= 1 and stats[0]["resigned"] + stats[0]["holdout_games"] <= 6
    assert decisions < probe[1] and samples < probe[3]


# ---- 5. the setter's contract -----------------------------------------------------------------------------------------------------
def test_argument_errors():
    P = pkg()
    eng = P.Engine(2, blocks=1, sims=4, dtype=P.NET_F32, threads=2)
    L = eng.L
    assert L.azr_selfplay_set_resign(None, -0.9, 2, 0.1, 0) == 3                 # AZR_E_BAD_HANDLE
    assert L.azr_selfplay_resign_stats(None, None) == 3 and L.azr_selfplay_resign_state(None, None, None, None) == 3
    assert L.azr_debug_resign(None, -0.9, 2, 0.1, 0, None, None, None, None, None, 0, None, None, None) == 3
    nan = float("nan")
    for args, why in (((nan, 2, 0.1), "must be numbers"), ((-0.9, 2, nan), "must be numbers"), ((nan, 0, 0.1), "must be numbers"),
                      ((-0.9, 0, nan), "must be numbers"), ((-1.5, 2, 0.1), "q_resign must lie in [-1, 1]"),
                      ((1.5, 2, 0.1), "q_resign must lie in [-1, 1]"), ((-0.9, 256, 0.1), "streak must be at most 255"),
                      ((-0.9, 2, -0.1), "holdout_share must lie in [0, 1]"), ((-0.9, 2, 1.5), "holdout_share must lie in [0, 1]")):
        with pytest.raises(P.AzrError) as e:
            eng.selfplay_set_resign(*args)
        assert e.value.code == 1 and "azr_selfplay_set_resign" in str(e.value) and why in str(e.value), (args, str(e.value))
    # off takes any numbers; on takes the ends of the ranges
    eng.selfplay_set_resign(-7.0, 0, 3.0); eng.selfplay_set_resign(-7.0, -1, -3.0)
    eng.selfplay_set_resign(-1.0, 1, 0.0); eng.selfplay_set_resign(1.0, 255, 1.0, 0xFFFFFFFF); eng.selfplay_set_resign(0.0, 0, 0.0)
    q, has, pl = np.array([-0.5], f32), np.ones(1, np.uint8), np.zeros(1, np.uint8)
    for args, why in (((0.0, 0, 0.0), "streak must lie in [1, 255]"), ((0.0, 256, 0.0), "streak must be at most 255"),
                      ((nan, 1, 0.0), "must be numbers"), ((0.0, 1, 1.5), "holdout_share must lie in [0, 1]")):
        with pytest.raises(P.AzrError) as e:
            eng.debug_resign(*args, 0, q, has, pl, [1], [1])
        assert e.value.code == 1 and "azr_debug_resign" in str(e.value) and why in str(e.value), (args, str(e.value))
    assert L.azr_debug_resign(eng.h, 0.0, 1, 0.0, 0, None, None, None, None, None, 1, None, None, None) == 1
    assert L.azr_selfplay_resign_stats(eng.h, None) == 1 and L.azr_selfplay_resign_state(eng.h, None, None, None) == 1
    row, who, hold = eng.debug_resign(0.0, 1, 1.0, 0, q, has, pl, [1], [1])
    assert (row[0], who[0], hold[0]) == (0, 0, True)
    eng.close()


def test_off_after_create_and_a_running_self_play_never_sees_a_change():
    run = _run(2)
    games, _ = SR.cached("retrace", run)
    series = [_series(g) for g in games]
    q_resign = _q_resign(series, 1)
    never, c0 = SR.cached("selfplay", run)

    def meddle(i, eng):
        if i == 0:                                                   # on while it runs
            assert eng.counters()["games_finished"] < QUOTA
            eng.selfplay_set_resign(q_resign, 1, 0.0, RSEED)
        st = eng.selfplay_resign_state()                             # ... is not in force: nothing to report
        assert not st[0].any() and (st[1] == RS.NONE).all() and not st[2].any()

    eng = SR.selfplay(run)                                           # the setter is never called before the start
    st = eng.selfplay_resign_state()
    assert not st[0].any() and (st[1] == RS.NONE).all() and not st[2].any()
    recs, c = SR.play_out(eng, QUOTA, 16, 400, after_run=meddle)
    assert recs.tobytes() == never.tobytes() and c == c0
    assert eng.selfplay_resign_stats() == dict(resigned=0, holdout_games=0, holdout_would_resign=0, holdout_not_lost=0)
    # the next start reads the setting, and resets the statistics with the counters
    SR.place(eng, run)
    again, c = SR.play_out(eng, QUOTA, 16, 400)
    stats = eng.selfplay_resign_stats()
    SR.place(eng, run)
    assert eng.selfplay_resign_stats() == dict(resigned=0, holdout_games=0, holdout_would_resign=0, holdout_not_lost=0)
    eng.close()
    on, c1, stats1 = _play(run, q_resign, 1)
    assert on.tobytes() != never.tobytes() and stats1["resigned"] >= 1
    assert again.tobytes() == on.tobytes() and c == c1 and stats == stats1
