"""GPU: the arena's dropped-game path (azr_arena.hpp, `if (fail)`): a game that ends in a rules error is dropped and the slot goes on.
RandomPlayer against RandomPlayer without yield reaches it by itself — reinforcement with every owned land full, where the reference's
pickRandomMove throws — and the oracle's _drop series (oracle/azr_oracle.h "a stopped game", tests/test_oracle_dropped_game.py) say
what the engine has to leave behind: the error count, the six result numbers, the per-slot log, the RNG stream, the record ring."""
import numpy as np
import pytest

import azr_testlib as T
import rules_settings as RS
from gpu_common import arena_play as play, assert_one_hot, half_slot, pkg, run_arena

pytestmark = pytest.mark.gpu
FM = T.data_field_mask()
ALL_STOP = dict(allow_yield=0, max_game_rounds=400)
MIX = dict(allow_yield=0, max_game_rounds=150)
RANDOM = 2


def six(res):
    return (res["count"], res["draw"], res["win"][0], res["win_and_started"][0], res["win"][1], res["win_and_started"][1])


def oracle_halves(G, per_slot, base, cfg, **kw):
    return [T.orc_play_half_games_drop(RANDOM, RANDOM, per_slot, *half_slot(g, G, base), cfg, **kw) for g in range(G)]


def compare_halves(eng, res, log, slots, per_slot):
    n, st, rd, fin = log
    assert (n == per_slot).all()   # a stopped pair is passed over: the slot's count moves on
    for g, o in enumerate(slots):
        for k in range(per_slot):
            if o["status"][k] == T.ORC_STOPPED:
                continue
            assert st[g, k] == o["status"][k] and rd[g, k] == o["rounds"][k], (g, k)
            assert (fin[g, k][FM] == o["finals"][k][FM]).all(), (g, k)
    assert eng.counters()["errors"] == sum(o["stops"] for o in slots)
    assert six(res) == tuple(np.sum([o["results"] for o in slots], axis=0))
    assert (eng.get_rng() == np.array([o["rng"] for o in slots], np.uint32)).all()


def test_concurrent_halves_every_game_stops(orc):
    """32 slots x 4 pairs, 400 rounds without yield: every game stops.  Nothing is counted, every slot has passed its four pairs, the
    streams stand where the stops left them, and the arena ends within run_arena's pass bound.
    On an MI355X 0.06 s."""
    P = pkg()
    G, per_slot, base = 32, 4, 4000
    slots = oracle_halves(G, per_slot, base, T.default_settings(**ALL_STOP))
    assert sum(o["stops"] for o in slots) == G * per_slot and all(o["last_error"] == 1 for o in slots)
    eng = P.Engine(G, blocks=1, sims=1, dtype=P.NET_F32, node_capacity=64, **ALL_STOP)
    res, log = run_arena(eng, RANDOM, RANDOM, 10 ** 6, per_slot, P.MIRROR_CONCURRENT, base)
    assert eng.counters()["errors"] == G * per_slot and res["count"] == 0 and six(res) == (0,) * 6
    compare_halves(eng, res, log, slots, per_slot)
    # the quota form: 64 games = 32 pairs over 16 slot pairs, two each, all of them stopped
    res, (n, _, _, _) = run_arena(eng, RANDOM, RANDOM, 64, 0, P.MIRROR_CONCURRENT, base)
    assert res["count"] == 0 and (n == 2).all()
    eng.close()


def test_concurrent_halves_stops_and_finishes(orc):
    """the same at 150 rounds: about half of the games stop, the others finish (some of them at round 151)
    On an MI355X 0.05 s."""
    P = pkg()
    G, per_slot, base = 32, 4, 4000
    slots = oracle_halves(G, per_slot, base, T.default_settings(**MIX))
    stops, done = sum(o["stops"] for o in slots), sum(o["results"][0] for o in slots)
    assert stops >= 32 and done >= 32 and stops + done == G * per_slot
    eng = P.Engine(G, blocks=1, sims=1, dtype=P.NET_F32, node_capacity=64, **MIX)
    res, log = run_arena(eng, RANDOM, RANDOM, 10 ** 6, per_slot, P.MIRROR_CONCURRENT, base)
    compare_halves(eng, res, log, slots, per_slot)
    eng.close()


@pytest.mark.parametrize("mirror", [True, False])
def test_sequential_slots_with_a_cap_go_on_after_a_stop(orc, mirror):
    """32 slots with a cap of 4 games at the five-switch setting: about one series in eight meets a stop and starts a fresh pair with
    player 0, so that it ends with 4 or 5 finished games.  Per slot the finished games' status, rounds and final states, the six result
    numbers, the error count and the stream's position.  The quota is 16 games a slot: no slot of this input comes near it, and a
    slot that went round in circles would use it up and fail the comparison instead of hanging the test.
    On an MI355X 0.04 s."""
    P = pkg()
    G, cap, base = 32, 4, 555
    cfg = T.default_settings(**RS.FIVE)
    slots = [T.orc_play_games_drop(RANDOM, RANDOM, cap, mirror, base + g, cfg, max_stops=4) for g in range(G)]
    assert all(o["rc"] == 0 for o in slots) and sum(o["stops"] for o in slots) >= 2
    assert {o["games"] for o in slots} == {cap, cap + 1}
    eng = P.Engine(G, blocks=1, sims=1, dtype=P.NET_F32, node_capacity=64, **RS.FIVE)
    res, (n, st, rd, fin) = run_arena(eng, RANDOM, RANDOM, 16 * G, cap, mirror, base)
    for g, o in enumerate(slots):
        k = o["games"]
        assert n[g] == k, (g, n[g], k)
        assert (st[g, :k] == o["status"][:k]).all() and (rd[g, :k] == o["rounds"][:k]).all(), g
        assert (fin[g, :k][:, FM] == o["finals"][:k][:, FM]).all(), g
    assert eng.counters()["errors"] == sum(o["stops"] for o in slots)
    assert six(res) == tuple(np.sum([o["results"] for o in slots], axis=0))
    assert (eng.get_rng() == np.array([o["rng"] for o in slots], np.uint32)).all()
    eng.close()


@pytest.mark.parametrize("kinds,mirror,seed,error", [((2, 1), True, 777, 1), ((2, 1), True, 1038, 2), ((2, 1), False, 1038, 2),
                                                     ((1, 1), True, 736, 2), ((1, 1), False, 813, 2)])
def test_script_side_series_go_on_after_a_stop(orc, kinds, mirror, seed, error):
    """A ScriptPlayer in a series that meets a stop (tests/test_oracle_dropped_game.py SCRIPT_STOPS; 400 rounds without yield): four
    slots around the stopping seed, a cap of 4 games.  With error class 2 it is the ScriptPlayer itself that stops, in the middle of
    its turn.  The player is not made anew for the next deal, so the games after the stop are the oracle's only if its memory (the
    land-set order, the attack target and source) went on as the oracle's did; the stream's position is compared as well.
    On an MI355X 0.01 s a case."""
    P = pkg()
    G, cap, base = 4, 4, seed - 1
    cfg = T.default_settings(**ALL_STOP)
    slots = [T.orc_play_games_drop(kinds[0], kinds[1], cap, mirror, base + g, cfg, max_stops=4) for g in range(G)]
    assert all(o["rc"] == 0 for o in slots) and slots[1]["stops"] == 1 and slots[1]["last_error"] == error
    eng = P.Engine(G, blocks=1, sims=1, dtype=P.NET_F32, node_capacity=64, **ALL_STOP)
    res, (n, st, rd, fin) = run_arena(eng, kinds[0], kinds[1], 16 * G, cap, mirror, base)
    for g, o in enumerate(slots):
        k = o["games"]
        assert n[g] == k, (g, n[g], k)
        assert (st[g, :k] == o["status"][:k]).all() and (rd[g, :k] == o["rounds"][:k]).all(), g
        assert (fin[g, :k][:, FM] == o["finals"][:k][:, FM]).all(), g
    assert eng.counters()["errors"] == sum(o["stops"] for o in slots)
    assert six(res) == tuple(np.sum([o["results"] for o in slots], axis=0))
    assert (eng.get_rng() == np.array([o["rng"] for o in slots], np.uint32)).all()
    eng.close()


# ---- the record ring -----------------------------------------------------------------------------------------------------------------
SCAP = 8192   # a 150-round game of two RandomPlayers records about 26 moves a round


def records_are_the_finished_games(rec, slots):
    """the drained records are the oracle's records of the finished games, each game one contiguous block, and nothing else"""
    blob = rec.tobytes()
    total = 0
    for g, o in enumerate(slots):
        for k, game in enumerate(o["records"]):
            assert len(game) == 0 or game.tobytes() in blob, (g, k)
            total += len(game)
    assert total == len(rec) == sum(o["nrec"] for o in slots)


@pytest.mark.parametrize("form", ["concurrent", "sequential"])
def test_a_dropped_game_leaves_the_record_ring_whole(orc, form):
    """Scripted collection on (the train-script form of tests/test_gpu_scripted_samples.py), two RandomPlayers at 150 rounds without
    yield: the drained records are byte for byte the oracle's records of the finished games (its RandomPlayer records are pinned to the
    reference's by tests/test_oracle_dropped_game.py), none of a stopped game, nothing dropped.
    The ring came back whole: a game is dealt only once its SCAP records are claimed and the ring holds G x SCAP, so if a dropped game
    kept its claim, the run's stops (more than G of them in either form) would leave no room for any deal, every slot would wait for a
    drain that frees nothing, and play()'s bound on runs would fail the test.  arena_start clears the claims, so this can be shown
    inside a run only; the run that follows on the same handle deals one game in every slot at once, the whole ring, after the drops.
    (The two-net form has no Script or Random side that could stop: an AlphaZero player's moves come from the legal mask.)
    On an MI355X 0.7 s (concurrent, 193 000 records) and 0.4 s."""
    P = pkg()
    cfg = T.default_settings(**MIX)
    if form == "concurrent":
        G, per_slot, base, mirror, total = 32, 4, 4000, P.MIRROR_CONCURRENT, 10 ** 6
        slots = oracle_halves(G, per_slot, base, cfg, scripted=True, rec_cap=4 * SCAP)
    else:
        G, per_slot, base, mirror, total = 16, 2, 555, P.MIRROR_SEQUENTIAL, 16 * 64
        slots = [T.orc_play_games_drop(RANDOM, RANDOM, per_slot, True, base + g, cfg, scripted=True, max_stops=16, rec_cap=4 * SCAP)
                 for g in range(G)]
        assert all(o["rc"] == 0 for o in slots)
    stops = sum(o["stops"] for o in slots)
    assert stops > G and sum(o["results"][0] for o in slots) >= G
    eng = P.Engine(G, blocks=1, sims=1, dtype=P.NET_F32, node_capacity=64, sample_capacity=SCAP, **MIX)
    res, (n, st, rd, fin), rec, _ = play(eng, RANDOM, RANDOM, total, per_slot, mirror, base, script=True)
    cn = eng.counters()
    assert cn["errors"] == stops and cn["records_dropped"] == 0 and cn["samples"] == len(rec)
    assert six(res) == tuple(np.sum([o["results"] for o in slots], axis=0))
    assert_one_hot(rec)
    records_are_the_finished_games(rec, slots)
    # one game in every slot at once (pairs base2 .. base2 + G/2 - 1, both halves): G x SCAP claims = the ring
    base2 = base + 1000
    one = oracle_halves(G, 1, base2, cfg, scripted=True, rec_cap=SCAP)
    res2, (n2, _, _, _), rec2, _ = play(eng, RANDOM, RANDOM, G, 0, P.MIRROR_CONCURRENT, base2, script=True)
    cn2 = eng.counters()
    assert (n2 == 1).all() and cn2["records_dropped"] == 0
    assert six(res2) == tuple(np.sum([o["results"] for o in one], axis=0))
    records_are_the_finished_games(rec2, one)
    eng.close()
