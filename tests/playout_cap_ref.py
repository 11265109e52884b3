"""Self-play with a playout cap, composed from the oracle's pieces (TEST INFRASTRUCTURE).

The oracle's orc_selfplay_game spends cfg.mcts_simulations on every decision and records every decision.  This module restates the
cap's coin from include/azr.h in Python integers and composes orc_selfplay_game's loop (alphazero_trainer.cpp:80-119) from the
oracle's exported pieces — orc_mcts_create, orc_mcts_simulate, orc_mcts_policy, orc_pick_highest, orc_pick_random, orc_encode,
orc_make_move, orc_game_status, orc_update_values — with the budget set per decision and the record written on full decisions only.

The oracle's search reads its budget from the orc_settings COPY at the start of struct orc_mcts (oracle/azr_oracle.c: `struct orc_mcts
{ orc_settings cfg; ...`, filled by orc_mcts_create), so selfplay_game writes mcts_simulations through a view of the tree object as
OrcSettings before each orc_mcts_simulate; right after creating the tree it asserts that the view reads back the settings it was
created from.

tests/test_playout_cap_ref.py pins the composition to orc_selfplay_game (full_prob = 1) and checks the gating on the CPU."""
import ctypes as C

import numpy as np

import azr_testlib as T

NOT_ENDED = -1
M32 = 0xFFFFFFFF


def mix(x):
    """azr_noise.hpp's noise_mix, as include/azr.h states it"""
    x &= M32
    x ^= x >> 16; x = (x * 0x7FEB352D) & M32
    x ^= x >> 15; x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def threshold(full_prob):
    """(uint32_t)(full_prob * 16777216.0f), in float"""
    return int(np.float32(full_prob) * np.float32(16777216.0))


def coin(full_prob, cap_seed, game_seed, decision):
    """True = decision `decision` of the game with seed `game_seed` is full"""
    if full_prob >= 1.0:
        return True
    k = mix(cap_seed + 0xC2B2AE35)
    k = mix(k ^ (game_seed & M32))
    k = mix(((k ^ (decision & M32)) + 0x27D4EB2F) & M32)
    return (k >> 8) < threshold(full_prob)


def coin_grid(full_prob, cap_seed, game_seeds, decisions):
    """the coin for every (game seed, decision) pair, vectorised: uint8 [len(game_seeds), len(decisions)]"""
    def vmix(x):
        x = x.astype(np.uint64)
        x ^= x >> np.uint64(16); x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
        x ^= x >> np.uint64(15); x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
        x ^= x >> np.uint64(16)
        return x
    s = np.asarray(game_seeds, np.uint64)[:, None]
    d = np.asarray(decisions, np.uint64)[None, :]
    k = np.uint64(mix(cap_seed + 0xC2B2AE35))
    k = vmix(k ^ s)
    k = vmix(((k ^ d) + np.uint64(0x27D4EB2F)) & np.uint64(M32))
    if full_prob >= 1.0:
        return np.ones(k.shape, np.uint8)
    return ((k >> np.uint64(8)) < np.uint64(threshold(full_prob))).astype(np.uint8)


def _same_settings(a, b):
    return all(getattr(a, f) == getattr(b, f) for f, _ in T.OrcSettings._fields_)


def selfplay_game(cfg, seed, eval_fn, full_prob, fast_simulations, cap_seed, cap=4096):
    """one self-play game under a playout cap.  Returns (records [n, 265] of the full decisions with z filled in, kinds [decisions]
    uint8 (1 = full), status, simulations the tree counted).  full_prob >= 1 or fast_simulations <= 0: no cap."""
    L = T.oracle()
    on = full_prob < 1.0 and fast_simulations > 0
    r = T.OrcRng()
    L.orc_rng_seed(C.byref(r), seed)
    m = L.orc_mcts_create(C.byref(cfg))
    view = C.cast(C.c_void_p(m), C.POINTER(T.OrcSettings))
    created = T.OrcSettings.from_buffer_copy(cfg)
    created.mcts_threads = min(max(created.mcts_threads, 1), 8)   # orc_mcts_create clamps its copy's thread count
    assert _same_settings(view.contents, created), "the tree object does not begin with its orc_settings copy"
    s = T.OrcState()
    L.orc_new_game(C.byref(s), C.byref(r))
    gs = NOT_ENDED
    recs, players, kinds = [], [], []
    try:
        d = 0
        while gs == NOT_ENDED:
            full = coin(full_prob, cap_seed, seed, d) if on else True
            view.contents.mcts_simulations = cfg.mcts_simulations if full else fast_simulations
            rc = L.orc_mcts_simulate(m, C.byref(s), C.byref(r), eval_fn, None)
            assert rc == 0, rc
            pi = np.zeros(43, np.float32)
            rc = L.orc_mcts_policy(m, C.byref(s), T.ptr(pi))
            assert rc == 0, rc
            li = L.orc_pick_highest(T.ptr(pi)) if s.round > cfg.temperature_threshold else L.orc_pick_random(T.ptr(pi), C.byref(r))
            if full and len(recs) < cap:
                rec = np.zeros(265, np.uint8)
                rec[0] = s.cur
                L.orc_encode(C.byref(s), T.ptr(rec[1:89]))
                rec[93:265] = pi.view(np.uint8)
                recs.append(rec)
                players.append(s.cur)
            kinds.append(1 if full else 0)
            rc = L.orc_make_move(C.byref(s), li, C.byref(r), C.byref(cfg))
            assert rc == 0, rc
            gs = L.orc_game_status(C.byref(s), C.byref(cfg))
            d += 1
        n = len(recs)
        pl = np.array(players if n else [0], np.int8)
        z = np.zeros(max(n, 1), np.float32)
        L.orc_update_values(T.ptr(pl), n, gs, T.ptr(z))
        for rec, zi in zip(recs, z):
            rec[89:93] = np.array([zi], np.float32).view(np.uint8)
        sims = int(L.orc_mcts_sim_count(m))
    finally:
        L.orc_mcts_destroy(m)
    return np.array(recs, np.uint8).reshape(n, 265), np.array(kinds, np.uint8), gs, sims


def oracle_game(cfg, seed, eval_fn, cap=4096):
    """orc_selfplay_game itself: (records [n, 265], status, simulations)"""
    L = T.oracle()
    buf = np.zeros((cap, 265), np.uint8)
    st, rounds = C.c_int(0), C.c_int(0)
    sims, evals = C.c_uint64(0), C.c_uint64(0)
    n = L.orc_selfplay_game(C.byref(cfg), seed, eval_fn, None, T.ptr(buf), cap, C.byref(st), C.byref(rounds), None, 0, C.byref(sims), C.byref(evals))
    assert 0 < n < cap
    return buf[:n].copy(), st.value, sims.value
