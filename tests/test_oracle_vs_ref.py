"""Live pinning of the oracle against the REAL reference (oracle/_ref/libazr_ref.so, compiled from
/root/reference by oracle/Makefile).  Skipped where oracle/_ref is absent."""
import ctypes as C
import os

import numpy as np
import pytest

import azr_testlib as T
import rules_settings as RS

pytestmark = [pytest.mark.ref, pytest.mark.skipif(not T.have_ref(), reason="oracle/_ref not built")]
FM = T.data_field_mask()


def test_bulk_random_games_bit_exact(orc):
    steps = 0
    for seed in range(1000, 11000):   # SURVEY §7 gate 2: >= 10 k seeded games, every state / mask / move / outcome
        g = T.ref_random_game(seed)
        h = T.orc_random_game(seed)
        assert len(g["moves"]) == len(h["moves"]), seed
        assert (g["moves"] == h["moves"]).all(), seed
        assert (g["masks"] == h["masks"]).all(), seed
        assert (g["states"][:, FM] == h["states"][:, FM]).all(), seed
        assert g["status"] == h["status"] and (g["final"][FM] == h["final"][FM]).all()
        steps += len(g["moves"])
    assert steps > 3000000


@pytest.mark.parametrize("rules", [dict(allow_yield=0), dict(limit_reinforcement=0), dict(limit_attack=1),
                                   dict(max_game_rounds=40), dict(min_unit_move=1)])
def test_rule_switches(orc, rules):
    base = dict(allow_yield=1, limit_reinforcement=1, limit_attack=0, max_game_rounds=58, min_unit_move=3)
    base.update(rules)
    R = T.ref()
    R.ref_set_rules(base["allow_yield"], base["limit_reinforcement"], base["limit_attack"], base["max_game_rounds"],
                    base["min_unit_move"])
    try:
        cfg = T.default_settings(**base)
        for seed in range(50, 90):
            g = T.ref_random_game(seed)
            h = T.orc_random_game(seed, cfg=cfg)
            assert len(g["moves"]) == len(h["moves"]) and (g["moves"] == h["moves"]).all(), (rules, seed)
            assert (g["masks"] == h["masks"]).all() and g["status"] == h["status"]
            assert (g["final"][FM] == h["final"][FM]).all()
    finally:
        R.ref_set_rules(1, 1, 0, 58, 3)


def test_encode_bit_exact(orc):
    R = T.ref()
    s = T.OrcState()
    for seed in (5, 6, 7):
        g = T.ref_random_game(seed)
        for st in g["states"][::3]:
            a = np.zeros(88, np.uint8); b = np.zeros(88, np.uint8)
            R.ref_encode(T.ptr(st), T.ptr(a))
            orc.orc_state_unpack(C.byref(s), T.ptr(st))
            orc.orc_encode(C.byref(s), T.ptr(b))
            assert (a == b).all()


def test_invert_players(orc):
    R = T.ref()
    s = T.OrcState()
    g = T.ref_random_game(11)
    for st in g["states"][::9]:
        a = st.copy()
        R.ref_invert_players(T.ptr(a))
        orc.orc_state_unpack(C.byref(s), T.ptr(st))
        orc.orc_invert_players(C.byref(s))
        b = np.zeros(160, np.uint8)
        orc.orc_state_pack(C.byref(s), T.ptr(b))
        assert (a[FM] == b[FM]).all()


DEFAULT_RULES = dict(allow_yield=1, limit_reinforcement=1, limit_attack=0, max_game_rounds=58, min_unit_move=3)


def ref_rules(**kw):
    r = dict(DEFAULT_RULES, **kw)
    T.ref().ref_set_rules(r["allow_yield"], r["limit_reinforcement"], r["limit_attack"], r["max_game_rounds"], r["min_unit_move"])


@pytest.mark.parametrize("kw", RS.SETTINGS, ids=RS.setting_id)
def test_lockstep_settings(orc, kw):
    """the games of the lock-step tests off the defaults (tests/rules_settings.py, the combination of all five switches among them):
    moves, masks, every state, outcome"""
    ref_rules(**kw)
    try:
        for seed, h in zip(RS.seeds(kw), RS.oracle_games(kw)):
            g = T.ref_random_game(int(seed), cap=65536)
            assert len(g["moves"]) == len(h["moves"]) and (g["moves"] == h["moves"]).all(), seed
            assert (g["masks"] == h["masks"]).all() and g["status"] == h["status"], seed
            assert (g["states"][:, FM] == h["states"][:, FM]).all() and (g["final"][FM] == h["final"][FM]).all(), seed
    finally:
        ref_rules()


@pytest.mark.parametrize("mum", [1, 5])
def test_every_move_index_under_min_unit_move(orc, mum):
    """the sweep of tests/test_gpu_rules.py::test_every_move_index_off_the_defaults_vs_oracle: each of the 44 indices on its states
    (saturated ones among them), return class and next state"""
    R = T.ref()
    cfg = T.default_settings(min_unit_move=mum)
    s, r, d = T.OrcState(), T.OrcRng(), np.zeros(160, np.uint8)
    ref_rules(min_unit_move=mum)
    try:
        for i, st in enumerate(RS.sweep_states()):
            for mv in range(44):
                a = st.copy()
                R.ref_seed(7000 + mv)
                rc = R.ref_make_move(T.ptr(a), mv)
                orc.orc_state_unpack(C.byref(s), T.ptr(st))
                r.x = 7000 + mv
                assert orc.orc_make_move(C.byref(s), mv, C.byref(r), C.byref(cfg)) == rc, (i, mv)
                if rc == 0:
                    orc.orc_state_pack(C.byref(s), T.ptr(d))
                    assert (a[FM] == d[FM]).all() and R.ref_rng_state() == r.x, (i, mv)
    finally:
        ref_rules()


def test_rng_states_that_play_does_not_reach(orc):
    """a die on the six raw values libstdc++ throws away, a float on the 62 it rounds up to 1.0f and clamps (for minstd_rand0 a seed
    is a state): value and the stream's position"""
    R = T.ref()
    r = T.OrcRng()
    for x in T.RNG_DIE_REJECT + T.RNG_FLOAT_CLAMP:
        R.ref_seed(x)
        r.x = x
        assert R.ref_rng_dice() == orc.orc_rng_dice(C.byref(r)) and R.ref_rng_state() == r.x, x
        R.ref_seed(x)
        r.x = x
        a, b = np.float32(R.ref_rng_float()), np.float32(orc.orc_rng_float(C.byref(r)))
        assert a.view(np.uint32) == b.view(np.uint32) and R.ref_rng_state() == r.x, x
        if x in T.RNG_FLOAT_CLAMP:
            assert a == np.nextafter(np.float32(1), np.float32(0))
    R.ref_seed(T.RNG_DIE_REJECT[0])
    assert R.ref_rng_dice() == 6 and R.ref_rng_state() == 2147382805   # two draws
    # the die branch inside attack moves: golden attack positions with the stream on the rejected states
    g = np.load(os.path.join(T.GOLDEN, "rules_games.npz"))
    idx = np.nonzero((g["states"][:, 149] == 3) & (g["moves"] != 42))[0][::97]
    cfg = T.default_settings()
    s, d = T.OrcState(), np.zeros(160, np.uint8)
    for k, i in enumerate(idx):
        x = (T.RNG_DIE_REJECT + [T.rng_step_back(y) for y in T.RNG_DIE_REJECT])[k % 12]
        a = g["states"][i].copy()
        R.ref_seed(x)
        assert R.ref_make_move(T.ptr(a), int(g["moves"][i])) == 0
        orc.orc_state_unpack(C.byref(s), T.ptr(g["states"][i]))
        r.x = x
        assert orc.orc_make_move(C.byref(s), int(g["moves"][i]), C.byref(r), C.byref(cfg)) == 0
        orc.orc_state_pack(C.byref(s), T.ptr(d))
        assert (a[FM] == d[FM]).all() and R.ref_rng_state() == r.x, i


@pytest.mark.parametrize("kinds", [(1, 2), (2, 1), (1, 1), (2, 2)])
def test_players_and_game_driver_bit_exact(orc, kinds):
    """ScriptPlayer / RandomPlayer / Game::playGames (mirrored pairs, alternating starts) against the real reference:
    results, every final state, round counts and the RNG stream position"""
    players_and_game_driver(kinds, range(100, 130), 8)


@pytest.mark.parametrize("kinds", [(1, 2), (2, 1), (1, 1)])
@pytest.mark.parametrize("kw", [dict(min_unit_move=1), dict(min_unit_move=5), dict(allow_yield=0, max_game_rounds=150)], ids=RS.setting_id)
def test_players_and_game_driver_off_the_defaults(orc, kinds, kw):
    """the same under the settings of tests/test_gpu_arena.py::test_script_and_random_players_arena_off_the_defaults and on its
    seeds (the harness's rule setter writes the SETTINGS object the players and Game read)"""
    ref_rules(**kw)
    try:
        players_and_game_driver(kinds, range(555, 555 + 32), 4, **kw)
    finally:
        ref_rules()


def players_and_game_driver(kinds, seeds, games, **kw):
    cfg = T.default_settings(**kw)
    for mirror in (1, 0):
        for seed in seeds:
            a = T.ref_play_games(kinds[0], kinds[1], games, mirror, seed)
            b = T.orc_play_games(kinds[0], kinds[1], games, mirror, seed, cfg=cfg)
            assert a[0] == b[0] and (a[1] == b[1]).all() and (a[2] == b[2]).all()
            assert (a[3][:, FM] == b[3][:, FM]).all() and a[4] == b[4]


@pytest.mark.parametrize("kinds", [(1, 2), (2, 1), (1, 1)])
def test_concurrent_halves_anchor_on_the_reference(orc, kinds):
    """AZR_MIRROR_CONCURRENT (include/azr.h): half 0 of the pair with seed q IS the first game a reference thread plays on a
    global engine seeded q (deal and dice from one stream) — results, final state, rounds, RNG position; half 1 is a game of its own
    (mirrored deal, player 1 starts, own dice stream) and a function of (q, half) alone."""
    for q in range(300, 320):
        a = T.ref_play_games(kinds[0], kinds[1], 1, 1, q)
        b = T.orc_play_half_games(kinds[0], kinds[1], 1, 0, q, 1)
        assert a[0] == b[0] and (a[1] == b[1]).all() and (a[2] == b[2]).all() and (a[3][:, FM] == b[3][:, FM]).all()
        h1 = T.orc_play_half_games(kinds[0], kinds[1], 1, 1, q, 1)
        h1b = T.orc_play_half_games(kinds[0], kinds[1], 3, 1, q - 14, 7)   # the same pair as the third game of another slot
        assert h1[0][0] == 1 and h1[1][0] == h1b[1][2] and (h1[3][0][FM] == h1b[3][2][FM]).all()
        assert h1[0][3] == 0 and h1[0][5] == h1[0][4]   # player 1 started: only its wins count as "won and started"
