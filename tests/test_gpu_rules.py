"""GPU parity, rules rows a1-a12: the wave-resident state-step kernels, called through the C-ABI,
against the oracle and the committed golden fixtures.  Bit-exact: states (160-B images incl. the derived
masks), legal masks, dice/RNG streams, outcomes, error classes, feature structs."""
import ctypes as C
import os

import numpy as np
import pytest

import azr_testlib as T
import rules_settings as RS
from gpu_common import pkg

pytestmark = pytest.mark.gpu
FM = T.data_field_mask()


def load(name):
    return np.load(os.path.join(T.GOLDEN, name))


def test_new_games_bit_exact(orc):
    G = 512
    eng = pkg().Engine(G, blocks=1, sims=1, dtype=pkg().NET_F32, node_capacity=64)
    seeds = np.concatenate([np.arange(1, G - 2, dtype=np.uint32), np.array([0, 2147483647, 4294967295], np.uint32)])
    eng.new_games(seeds)
    got, rng = eng.get_states(), eng.get_rng()
    s, r, d = T.OrcState(), T.OrcRng(), np.zeros(160, np.uint8)
    for g in range(G):
        orc.orc_rng_seed(C.byref(r), int(seeds[g]))
        orc.orc_new_game(C.byref(s), C.byref(r))
        orc.orc_state_pack(C.byref(s), T.ptr(d))
        assert (d == got[g]).all(), g
        assert r.x == rng[g]
    eng.close()


def lockstep(orc, seeds, on_move=None, **kw):
    """G games stepped to the end in lock-step under the settings kw; move choice = the oracle's randomMask on its own stream (exactly
    the golden generator's policy), dice = the device's per-game minstd_rand0 stream kept aligned with the oracle's.  Every state
    image, mask, status and RNG word is compared after every move.  on_move(OrcState, mask, move) sees each move before it is played.
    Returns (move lists, final statuses, final state images, the oracle's final states)."""
    cfg = T.default_settings(**kw)
    G = len(seeds)
    eng = pkg().Engine(G, blocks=1, sims=1, dtype=pkg().NET_F32, node_capacity=64, **kw)
    eng.new_games(seeds)
    S = [T.OrcState() for _ in range(G)]
    R = [T.OrcRng() for _ in range(G)]
    for g in range(G):
        orc.orc_rng_seed(C.byref(R[g]), int(seeds[g]))
        orc.orc_new_game(C.byref(S[g]), C.byref(R[g]))
    traj = [[] for _ in range(G)]
    d = np.zeros(160, np.uint8)
    steps = 0
    while True:
        status = eng.status()
        vm = eng.valid_moves()
        states = eng.get_states()
        moves = np.full(G, 255, np.uint8)
        rng = np.zeros(G, np.uint32)
        live = 0
        for g in range(G):
            st = orc.orc_game_status(C.byref(S[g]), C.byref(cfg))
            assert st == status[g], (g, steps)
            orc.orc_state_pack(C.byref(S[g]), T.ptr(d))
            assert (d == states[g]).all(), (g, steps)
            if st != -1:
                rng[g] = R[g].x
                continue
            live += 1
            m = orc.orc_valid_moves(C.byref(S[g]), C.byref(cfg))
            assert m == int(vm[g]), (g, steps, hex(m), hex(int(vm[g])))
            mv = int(orc.orc_random_mask(C.byref(R[g]), m)).bit_length() - 1
            if on_move:
                on_move(S[g], m, mv)
            moves[g] = mv
            traj[g].append(mv)
            rng[g] = R[g].x
        if live == 0:
            break
        eng.set_rng(rng)
        rc = eng.make_moves(moves)
        assert (rc == 0).all()
        for g in range(G):
            if moves[g] != 255:
                assert orc.orc_make_move(C.byref(S[g]), int(moves[g]), C.byref(R[g]), C.byref(cfg)) == 0
        assert (eng.get_rng()[moves != 255] == np.array([R[g].x for g in range(G)], np.uint32)[moves != 255]).all(), steps
        steps += 1
        assert steps < 5000
    out = traj, eng.status(), eng.get_states(), S
    eng.close()
    return out


def test_lockstep_random_games_vs_oracle_and_golden(orc):
    """the default settings, 256 games: the golden games and 236 more"""
    gold = load("rules_games.npz")
    seeds = np.concatenate([gold["seeds"], np.arange(3000, 3000 + 236, dtype=np.uint32)])
    traj, status, final, _ = lockstep(orc, seeds)
    # the first len(gold seeds) games are the golden ones: same move lists and outcomes as the REFERENCE produced
    for k in range(len(gold["seeds"])):
        lo, hi = gold["starts"][k], gold["starts"][k + 1]
        assert traj[k] == list(gold["moves"][lo:hi])
        assert status[k] == gold["status"][k]
        assert (final[k][FM] == gold["finals"][k][FM]).all()


@pytest.mark.parametrize("kw", RS.SETTINGS, ids=RS.setting_id)
def test_lockstep_random_games_under_settings(orc, kw):
    """The same lock-step comparison off the defaults (the oracle is pinned to the reference on these very games by
    tests/test_oracle_vs_ref.py::test_lockstep_settings): make_move, valid_moves, status and the dice under each run-time setting, 32 games
    from seed 3000 and the setting's extra seeds (tests/rules_settings.py).  The census of what these inputs reach is taken here, on the
    oracle's states, and has to hold what tests/test_rules_census.py requires of the setting: a lock-step run that never met a full
    land compares nothing of the clamps.
    On an MI355X 0.3 to 1.7 s a setting (the default test: 0.6 s)."""
    count = dict.fromkeys(RS.SITUATIONS, 0)

    def on_move(s, mask, mv):
        for k in RS.classify(s, mask, mv, kw):
            count[k] += 1

    traj, status, final, S = lockstep(orc, RS.seeds(kw), on_move, **kw)
    for g, game in enumerate(RS.oracle_games(kw)):   # the games the census test counted
        assert traj[g] == list(game["moves"]) and status[g] == game["status"], g
        for k in RS.classify_end(S[g], int(status[g]), kw):
            count[k] += 1
    assert count == RS.census(kw)
    short = {k: count[k] for k in RS.required(kw) if count[k] < RS.CENSUS_MIN}
    assert not short, short


def test_every_move_index_error_class_and_next_state():
    g = load("moves_all.npz")
    states = np.repeat(g["states"], 44, axis=0)
    moves = np.tile(np.arange(44, dtype=np.uint8), len(g["states"]))
    G = len(states)
    eng = pkg().Engine(G, blocks=1, sims=1, dtype=pkg().NET_F32, node_capacity=64)
    eng.set_states(states)
    # dice seed = base + move, as the generator seeded the reference's engine before each call
    seeds = (int(g["dice_seed_base"]) + moves.astype(np.uint32)) % 2147483647
    eng.set_rng(seeds.astype(np.uint32))
    rc = eng.make_moves(moves)
    after = eng.get_states()
    assert (rc.reshape(-1, 44) == g["rc"]).all()
    ok = (g["rc"] == 0).reshape(-1)
    assert (after[ok][:, FM] == g["next"].reshape(-1, 160)[ok][:, FM]).all()
    # a throwing move leaves the stored game untouched
    assert (after[~ok][:, FM] == states[~ok][:, FM]).all()
    eng.close()


def test_encode_status_and_roundtrip():
    g = load("encode.npz")
    G = len(g["states"])
    eng = pkg().Engine(G, blocks=1, sims=1, dtype=pkg().NET_F32, node_capacity=64)
    eng.set_states(g["states"])
    assert (eng.encode() == g["in88"]).all()
    assert (eng.status() == g["status"]).all()
    # import ignores the image's derived masks and export recomputes them: must reproduce the reference's
    assert (eng.get_states()[:, FM] == g["states"][:, FM]).all()
    eng.close()


def test_rule_switches_masks(orc):
    """legal masks under non-default LIMIT_* settings against the oracle (pinned to the reference in
    tests/test_oracle_vs_ref.py::test_rule_switches)"""
    g = load("rules_games.npz")
    states = g["states"][::7]
    G = len(states)
    s = T.OrcState()
    for kw in (dict(limit_reinforcement=0), dict(limit_attack=1), dict(allow_yield=0, max_game_rounds=40)):
        cfg = T.default_settings(**kw)
        eng = pkg().Engine(G, blocks=1, sims=1, dtype=pkg().NET_F32, node_capacity=64, **kw)
        eng.set_states(states)
        vm, st = eng.valid_moves(), eng.status()
        for i in range(G):
            orc.orc_state_unpack(C.byref(s), T.ptr(states[i]))
            assert orc.orc_valid_moves(C.byref(s), C.byref(cfg)) == int(vm[i])
            assert orc.orc_game_status(C.byref(s), C.byref(cfg)) == st[i]
        eng.close()


@pytest.mark.parametrize("mum", [1, 5])
def test_every_move_index_off_the_defaults_vs_oracle(orc, mum):
    """test_every_move_index_error_class_and_next_state with MIN_UNIT_MOVE 1 and 5, against the oracle (pinned for exactly this sweep
    by tests/test_oracle_vs_ref.py::test_every_move_index_under_min_unit_move): each of the 44 indices on about 100 states of all six
    phases from the 150- and 120-round games of tests/rules_settings.py, saturated ones among them — return class, next state, RNG
    word; a refused move leaves the stored game untouched.
    On an MI355X 0.03 s."""
    base = RS.sweep_states()
    assert set(base[:, 149]) == set(range(6)) and len(base) >= 96
    states = np.repeat(base, 44, axis=0)
    moves = np.tile(np.arange(44, dtype=np.uint8), len(base))
    G = len(states)
    seeds = (7000 + 13 * np.arange(G, dtype=np.uint32)) % 2147483647
    eng = pkg().Engine(G, blocks=1, sims=1, dtype=pkg().NET_F32, node_capacity=64, min_unit_move=mum)
    eng.set_states(states)
    eng.set_rng(seeds)
    rc = eng.make_moves(moves)
    after, rng = eng.get_states(), eng.get_rng()
    eng.close()
    cfg = T.default_settings(min_unit_move=mum)
    s, r, d = T.OrcState(), T.OrcRng(), np.zeros(160, np.uint8)
    classes = set()
    for i in range(G):
        orc.orc_state_unpack(C.byref(s), T.ptr(states[i]))
        r.x = int(seeds[i])
        want = orc.orc_make_move(C.byref(s), int(moves[i]), C.byref(r), C.byref(cfg))
        classes.add(want)
        assert rc[i] == want, (i // 44, int(moves[i]), int(rc[i]), want)
        if want == 0:
            orc.orc_state_pack(C.byref(s), T.ptr(d))
            assert (after[i] == d).all() and rng[i] == r.x, (i // 44, int(moves[i]))
        else:
            assert (after[i][FM] == states[i][FM]).all(), (i // 44, int(moves[i]))
    assert classes == {0, 1, 2}


# ---- the two RNG branches that play does not reach (azr_wave.hpp rng_downscale / rng_float) ------------------------------------------
def test_die_rejection_in_attack_moves(orc):
    """libstdc++'s uniform_int_distribution scales minstd_rand0's raw value down by (2^31 - 3) / 6 and draws again when the raw value
    is one of the six largest: 6 states in 2^31, which no game and no known-answer stream reaches.  Golden attack positions (phase
    attack, move not SKIP) with the stream placed on each of those states (azr_testlib.RNG_DIE_REJECT), and one step before each (the
    rejection then meets the second die), against orc_make_move: state and RNG word.
    On an MI355X 0.01 s."""
    g = load("rules_games.npz")
    idx = np.nonzero((g["states"][:, 149] == 3) & (g["moves"] != 42))[0]
    start = np.array(T.RNG_DIE_REJECT + [T.rng_step_back(x) for x in T.RNG_DIE_REJECT], np.uint32)
    idx = idx[:: len(idx) // (4 * len(start))][: 4 * len(start)]
    G = len(idx)
    states, moves, rng0 = g["states"][idx], g["moves"][idx], np.tile(start, 4)
    eng = pkg().Engine(G, blocks=1, sims=1, dtype=pkg().NET_F32, node_capacity=64)
    eng.set_states(states)
    eng.set_rng(rng0)
    assert (eng.make_moves(moves) == 0).all()
    after, rng = eng.get_states(), eng.get_rng()
    eng.close()
    cfg = T.default_settings()
    s, r, d = T.OrcState(), T.OrcRng(), np.zeros(160, np.uint8)
    for i in range(G):
        orc.orc_state_unpack(C.byref(s), T.ptr(states[i]))
        r.x = int(rng0[i])
        assert orc.orc_make_move(C.byref(s), int(moves[i]), C.byref(r), C.byref(cfg)) == 0
        orc.orc_state_pack(C.byref(s), T.ptr(d))
        assert (after[i][FM] == d[FM]).all() and rng[i] == r.x, i


def test_float_clamp_in_sampled_pick(orc):
    """rng_float rounds the 62 largest raw values up to 1.0f and clamps them to nextafterf(1, 0) (libstdc++'s generate_canonical):
    after a short host-stepped search (orc_hash_eval, 8 simulations) the stream is placed on clamp states and pick(sample=True) is
    compared with orc_pick_random on the same policy and state: move and RNG word.
    What this pins is that the branch takes one draw and picks the oracle's move.  It does not pin the clamped VALUE: the pick returns
    the first index whose running sum reaches sum * u, and for a search policy (entries k / N) u = 1.0f and u = nextafterf(1, 0) stop at
    the same index, the last non-zero entry; they would part only on an entry below one ulp of the sum, which no visit count gives.
    No call of the C-ABI hands rng_float's value out or takes a policy in, so the value itself is pinned on the oracle's side only
    (tests/test_oracle_golden.py::test_rng_states_that_play_does_not_reach, against the reference).
    On an MI355X 0.01 s."""
    stub = orc.orc_hash_eval
    stub.argtypes = [C.c_void_p, T.u8p, T.f32p, C.c_void_p]
    clamp = [T.RNG_FLOAT_CLAMP[i] for i in (0, 1, 17, 30, 44, 61)]
    states = np.load(os.path.join(T.GOLDEN, "rules_games.npz"))["states"][40::331][: len(clamp)].copy()
    G = len(states)
    eng = pkg().Engine(G, blocks=1, sims=8, dtype=pkg().NET_F32)
    eng.set_states(states)
    eng.set_rng(np.arange(900, 900 + G, dtype=np.uint32))
    assert (eng.status() == -1).all()
    T.engine_stub_search(eng, stub, 16)
    pi = eng.policy()
    eng.set_rng(np.array(clamp, np.uint32))
    moves = eng.pick(sample=True)
    rng = eng.get_rng()
    eng.close()
    r = T.OrcRng()
    for g in range(G):
        r.x = clamp[g]
        assert orc.orc_rng_float(C.byref(r)) == np.nextafter(np.float32(1), np.float32(0))
        r.x = clamp[g]
        assert orc.orc_pick_random(T.ptr(pi[g]), C.byref(r)) == moves[g], g
        assert r.x == rng[g], g
