"""CPU: the oracle's series functions that go on after a stopped game (oracle/azr_oracle.h, "a stopped game"), the checker of the
engine's dropped-game path (azr_arena.hpp, `if (fail)`; tests/test_gpu_dropped_game.py).  The C forms are compared with the slot loop
written out again here, in Python over the oracle's public turn and rules functions, for RandomPlayer against RandomPlayer: the input
that stops by itself (pickRandomMove on the empty set, reinforcement with every owned land full)."""
import ctypes as C

import numpy as np
import pytest

import azr_testlib as T
import rules_settings as RS

ALL_STOP = dict(allow_yield=0, max_game_rounds=400)
MIX = dict(allow_yield=0, max_game_rounds=150)


def _play_out(L, s, r, cfg):
    """Game::gameLoop for two RandomPlayers: (error class, status)"""
    while True:
        cur, setup = s.cur, s.phase == 0
        rc = L.orc_random_take_turn(C.byref(s), cur, C.byref(r), C.byref(cfg))
        if rc:
            return rc, None
        gs = -1 if setup else L.orc_game_status(C.byref(s), C.byref(cfg))
        if gs != -1:
            return 0, gs
        assert s.cur != cur


def _image(L, s):
    d = np.zeros(160, np.uint8)
    L.orc_state_pack(C.byref(s), T.ptr(d))
    return d


def slot_sequential(L, cfg, cap, mirror, seed, max_stops=64):
    r, s, prev = T.OrcRng(), T.OrcState(), T.OrcState()
    L.orc_rng_seed(C.byref(r), seed)
    games, stops, last, start, phase = [], 0, 0, 0, 0
    while not (phase == 0 and len(games) >= cap) and stops < max_stops:
        if mirror and start:
            C.memmove(C.byref(s), C.byref(prev), C.sizeof(s))
            L.orc_invert_players(C.byref(s))
        else:
            L.orc_new_game(C.byref(s), C.byref(r))
            C.memmove(C.byref(prev), C.byref(s), C.sizeof(s))
        s.cur = start
        rc, gs = _play_out(L, s, r, cfg)
        if rc:
            stops, last, start, phase = stops + 1, rc, 0, 0
            continue
        games.append((gs, s.round, _image(L, s), start))
        start, phase = start ^ 1, phase ^ 1
    return games, stops, last, r.x


def slot_half(L, cfg, games_n, half, q0, stride):
    r, s = T.OrcRng(), T.OrcState()
    games, stops, last = [], 0, 0
    for k in range(games_n):
        q = (q0 + k * stride) & 0xffffffff
        L.orc_rng_seed(C.byref(r), q)
        L.orc_new_game(C.byref(s), C.byref(r))
        if half:
            L.orc_invert_players(C.byref(s))
            L.orc_rng_seed(C.byref(r), (q + (1 << 30)) & 0xffffffff)
        s.cur = half
        rc, gs = _play_out(L, s, r, cfg)
        if rc:
            stops, last = stops + 1, rc
            games.append(None)
        else:
            games.append((gs, s.round, _image(L, s), half))
    return games, stops, last, r.x


def six(games):
    t = [0] * 6
    for g in games:
        if g is None:
            continue
        gs, _, _, start = g
        t[0] += 1
        t[1] += gs == -2
        for p in (0, 1):
            t[2 + 2 * p] += gs == p
            t[3 + 2 * p] += gs == p and start == p
    return tuple(t)


@pytest.mark.parametrize("kw", [RS.FIVE, MIX, dict(max_game_rounds=150)], ids=RS.setting_id)
@pytest.mark.parametrize("mirror", [True, False])
def test_sequential_slot_goes_on_as_written_out(orc, kw, mirror):
    cfg = T.default_settings(**kw)
    stops = over = 0
    for seed in range(555, 555 + 32):
        o = T.orc_play_games_drop(2, 2, 4, mirror, seed, cfg, max_stops=8)
        games, n_stop, last, rng = slot_sequential(orc, cfg, 4, mirror, seed, max_stops=8)
        assert (o["games"], o["stops"], o["last_error"], o["rng"]) == (len(games), n_stop, last, rng), seed
        assert o["results"] == six(games) and (o["rc"] != 0) == (n_stop >= 8), seed
        assert o["games"] in (4, 5) or o["rc"] != 0   # the cap is looked at before a pair only
        for k, (gs, rd, img, _) in enumerate(games):
            assert o["status"][k] == gs and o["rounds"][k] == rd and (o["finals"][k] == img).all(), (seed, k)
        stops += n_stop
        over += len(games) == 5
    assert stops > 0 and (over > 0 or kw is MIX)


@pytest.mark.parametrize("kw", [ALL_STOP, MIX, RS.FIVE], ids=RS.setting_id)
def test_concurrent_slot_goes_on_as_written_out(orc, kw):
    cfg = T.default_settings(**kw)
    G, per, base = 32, 4, 4000
    stops = fin = 0
    for g in range(G):
        o = T.orc_play_half_games_drop(2, 2, per, g & 1, base + (g >> 1), G // 2, cfg)
        games, n_stop, last, rng = slot_half(orc, cfg, per, g & 1, base + (g >> 1), G // 2)
        assert (o["rc"], o["games"], o["stops"], o["last_error"], o["rng"]) == (0, per, n_stop, last, rng), g
        assert o["results"] == six(games), g
        for k, game in enumerate(games):
            if game is None:
                assert o["status"][k] == T.ORC_STOPPED, (g, k)
            else:
                assert o["status"][k] == game[0] and o["rounds"][k] == game[1] and (o["finals"][k] == game[2]).all(), (g, k)
        stops += n_stop
        fin += o["results"][0]
    assert stops + fin == G * per and stops > 0
    if kw is ALL_STOP:   # every game stops in reinforcement with nothing left to reinforce: invalid_argument
        assert fin == 0 and last == 1
    else:
        assert fin > 0


@pytest.mark.parametrize("kinds", [(1, 2), (2, 1), (1, 1), (2, 2)])
def test_a_series_without_a_stop_is_the_plain_series(orc, kinds):
    """where nothing stops the _drop forms are orc_play_games2 / orc_play_half_games: the default settings, all player kinds"""
    for mirror in (True, False):
        for seed in (100, 101, 102):
            a = T.orc_play_games(kinds[0], kinds[1], 6, mirror, seed)
            o = T.orc_play_games_drop(kinds[0], kinds[1], 6, mirror, seed)
            assert o["rc"] == 0 and o["stops"] == 0 and o["games"] == 6
            assert a[0] == o["results"] and (a[1] == o["status"][:6]).all() and (a[2] == o["rounds"][:6]).all()
            assert (a[3] == o["finals"][:6]).all() and a[4] == o["rng"]
    for g in range(4):
        a = T.orc_play_half_games(kinds[0], kinds[1], 3, g & 1, 777 + (g >> 1), 2)
        o = T.orc_play_half_games_drop(kinds[0], kinds[1], 3, g & 1, 777 + (g >> 1), 2)
        assert o["stops"] == 0 and a[0] == o["results"] and (a[1] == o["status"]).all() and (a[3] == o["finals"]).all()


def test_the_plain_series_ends_at_the_stop(orc):
    """the reference's way: seeds 555, 556 and 557 of Random against Random without yield stop with invalid_argument"""
    cfg = T.default_settings(**ALL_STOP)
    res = T.OrcResults()
    for seed in (555, 556, 557):
        rc = orc.orc_play_games(C.byref(cfg), 2, 2, 4, 1, seed, None, None, C.byref(res), None, None, None)
        assert rc == 1 and res.count == 0


def test_a_stopped_game_leaves_no_records(orc):
    """RandomPlayer's one-hot records: those of the finished games only, each game's block closed with its z"""
    cfg = T.default_settings(**MIX)
    met = 0
    for g in range(8):
        o = T.orc_play_half_games_drop(2, 2, 4, g & 1, 4000 + (g >> 1), 4, cfg, scripted=True, rec_cap=40000)
        assert o["nrec"] == sum(len(r) for r in o["records"]) < 40000
        for k, rec in enumerate(o["records"]):
            if o["status"][k] == T.ORC_STOPPED:
                assert len(rec) == 0
                met += 1
                continue
            pi = rec[:, 93:265].copy().view(np.float32)
            z = rec[:, 89:93].copy().view(np.float32)[:, 0]
            assert len(rec) > 0 and ((pi == 1.0).sum(1) == 1).all() and ((pi != 0.0).sum(1) == 1).all()
            want = np.where(o["status"][k] == -2, 0.0, np.where(rec[:, 0] == o["status"][k], 1.0, -1.0))
            assert (z == want).all(), (g, k)
    assert met > 0


# series with a ScriptPlayer that meet a stop, 400 rounds without yield: (kinds, mirrored, slot seed, error class of the stop).  Class 2
# is the ScriptPlayer's own: attackLand finds no room for its reinforcement and throws in the middle of its turn.
SCRIPT_STOPS = [((2, 1), True, 777, 1), ((2, 1), True, 1038, 2), ((2, 1), False, 1038, 2), ((1, 1), True, 736, 2), ((1, 1), False, 813, 2)]


@pytest.mark.parametrize("kinds,mirror,seed,error", SCRIPT_STOPS)
def test_series_with_a_script_player_meet_a_stop(orc, kinds, mirror, seed, error):
    """the inputs of tests/test_gpu_dropped_game.py::test_script_side_series_go_on_after_a_stop do stop, once, with the class listed,
    and the slot then plays its games to the end; the plain series ends there with the same class"""
    cfg = T.default_settings(**ALL_STOP)
    o = T.orc_play_games_drop(kinds[0], kinds[1], 4, mirror, seed, cfg, max_stops=4)
    assert (o["rc"], o["stops"], o["last_error"]) == (0, 1, error) and o["games"] in (4, 5) and o["results"][0] == o["games"]
    res = T.OrcResults()
    assert orc.orc_play_games(C.byref(cfg), kinds[0], kinds[1], 6, int(mirror), seed, None, None, C.byref(res), None, None, None) == error


@pytest.mark.parametrize("key,random_player", [("12", 1), ("21", 0)])
def test_random_player_records_equal_the_reference_fixture(orc, key, random_player):
    """the oracle's RandomPlayer records are the reference's (tests/golden/scripted_samples.npz, one whole Script-vs-Random game in
    either seating): byte for byte the fixture game's records of the Random side"""
    import os
    f = np.load(os.path.join(T.GOLDEN, "scripted_samples.npz"))
    c, g, i = (int(v) for v in f["full_at_" + key])
    k0, k1, mirror, base = (int(v) for v in f["configs"][c])
    o = T.orc_play_games_drop(k0, k1, 4, bool(mirror), base + g, scripted=True, rec_cap=20000)
    full = f["full_" + key]
    want = full[full[:, 0] == random_player]
    assert o["stops"] == 0 and len(want) > 0
    assert o["records"][i].tobytes() == want.tobytes()
