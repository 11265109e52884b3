"""The proof every self-play option shares (TEST INFRASTRUCTURE, not collected): the four late golden games are played in device
self-play and retraced decision by decision through the host-stepped entry points (azr_mcts_*, azr_debug_*); the device's record stream
must hold every retraced game's records, bit for bit and side by side.  A Run names the games and the options in force; selfplay and
retrace take it; the option under test turns the retrace's arrays into the stream it expects with its own restatement (surprise_ref,
value_mix_ref) and hands it to assert_streams.  What a Run gave is computed once per process (cached); callers must not write into it.
Engines of one block, NET_F32; the weights are the Run's: make_net_flat(1, seed=11, perturb_bn=True), or the sharp net of that seed
(azr_testlib.make_sharp_net_flat: priors of exactly 0 and 1, often on illegal moves, and values of exactly +-1)."""
import os
from typing import NamedTuple, Optional, Tuple

import numpy as np

import azr_testlib as T
import playout_cap_ref as R
from gpu_common import pkg

f32 = np.float32
G = 8


class Run(NamedTuple):
    """the games of seeds base .. base + quota - 1 from late_positions() and the self-play options in force (None: the setter is never
    called).  surprise and value_mix only rewrite the written records: retrace does not look at them"""
    base: int
    quota: int
    threads: int
    sims: int
    fast: int = 0
    cap: Optional[Tuple[float, int]] = None               # (full_prob, cap_seed), the fast budget is `fast`
    dirichlet: Optional[Tuple[float, int]] = None         # (alpha, noise_seed)
    forced: Optional[Tuple[float, bool]] = None           # (k, prune)
    surprise: Optional[Tuple[float, float, int]] = None   # (share, max_weight, seed)
    value_mix: Optional[float] = None                     # q_share
    net: str = "base"                                     # the weights: a key of NETS


class Game(NamedTuple):
    """one retraced game, a row per recorded (full) decision: the 265-byte records with the bare z, z, the legal moves, and the root's
    N, Q and prior of azr_mcts_root_stats"""
    records: np.ndarray
    z: np.ndarray
    valid: np.ndarray
    N: np.ndarray
    Q: np.ndarray
    prior: np.ndarray


def late_positions(slots=G):
    """four running positions 20 and 10 moves before the end of golden games that reach the last rounds: the games end soon"""
    gold = np.load(os.path.join(T.GOLDEN, "rules_games.npz"))
    ends = gold["starts"][1:]
    idx = [ends[3] - 20, ends[13] - 20, ends[19] - 20, ends[3] - 10]
    states = np.concatenate([gold["states"][idx], gold["states"][idx]]).copy()   # slots 4..7 idle under the quota
    return states, np.arange(600, 600 + slots, dtype=np.uint32)


NETS = {"base": lambda: T.make_net_flat(1, seed=11, perturb_bn=True), "sharp": lambda: T.make_sharp_net_flat(1, seed=11)}


def engine(threads, sims, slots=G, net="base", **settings):
    P = pkg()
    eng = P.Engine(slots, blocks=1, sims=sims, dtype=P.NET_F32, threads=threads, **settings)
    eng.set_weights(NETS[net]())
    return eng


def play_out(eng, quota, passes, runs, after_run=None, exact=True):
    """a started self-play until `quota` games are over, drained after every run of `passes` passes; after_run(i, eng) is called between
    run i and its drain.  exact = False: a self-play without a quota, which plays on past `quota`.  (records, counters)"""
    recs = []
    for i in range(runs):
        eng.selfplay_run(passes)
        if after_run:
            after_run(i, eng)
        recs.append(eng.drain())
        c = eng.counters()
        if c["games_finished"] + c["errors"] >= quota:
            break
    c = eng.counters()
    assert c["games_finished"] == quota or (not exact and c["games_finished"] > quota), c
    assert c["errors"] == 0 and c["nodes_dropped"] == 0 and c["records_dropped"] == 0, c
    return np.concatenate(recs), c


def place(eng, run):
    """the late positions and their RNG streams, and the quota started from them"""
    states, rngs = late_positions()
    eng.set_states(states)
    eng.set_rng(rngs)
    eng.selfplay_start_games_from_states(run.base, run.quota)


def selfplay(run, configure=None):
    """a new engine with the run's options set, then configure(eng) for what the test itself does to the setters, started"""
    eng = engine(run.threads, run.sims, net=run.net)
    if run.dirichlet:
        eng.selfplay_set_dirichlet(*run.dirichlet)
    if run.forced:
        eng.selfplay_set_forced_playouts(*run.forced)
    if run.cap:
        eng.selfplay_set_playout_cap(run.cap[0], run.fast, run.cap[1])
    if run.surprise:
        eng.selfplay_set_surprise_weighting(*run.surprise)
    if run.value_mix is not None:
        eng.selfplay_set_value_mix(run.value_mix)
    if configure:
        configure(eng)
    place(eng, run)
    return eng


def outcome_z(status, player):
    """the bare z of a record of `player` in a game that ended with `status` (the winner, or -2: a draw)"""
    return 0.0 if status == -2 else (1.0 if player == status else -1.0)


def retrace(run):
    """the run's games through azr_mcts_*, one after the other in every slot (slot 0 is read).  Per decision: the kind by the cap's coin;
    with Dirichlet noise, forced playouts or a cap in force the vector of azr_debug_root_noise (or the constant: a fast decision, and
    every decision without Dirichlet noise), the factor and the budget of that kind (with none of them no setter is called); one search;
    the pruned policy into the record where the run prunes, the unpruned pick as the move.  ([Game], totals)"""
    eng = engine(run.threads, run.sims, net=run.net)
    states, rngs = late_positions()
    dnv, thr = f32(eng.settings.dir_noise_value), eng.settings.temperature_threshold
    k, prune = run.forced or (0.0, False)
    games, tot = [], dict(decisions=0, simulations=0, samples=0)
    for g in range(run.quota):
        eng.set_states(np.repeat(states[g:g + 1], G, 0))
        eng.set_rng(np.full(G, rngs[g], np.uint32))
        eng.mcts_clear()
        rows, d = [], 0
        while True:
            full = R.coin(run.cap[0], run.cap[1], run.base + g, d) if run.cap else True
            budget = run.sims if full else run.fast
            valid = eng.valid_moves()
            if run.dirichlet or run.forced or run.cap:
                sampled = full and run.dirichlet
                eta = eng.debug_root_noise(*run.dirichlet, [run.base + g], [d], valid[:1]) if sampled else np.full((1, 43), dnv, f32)
                eng.set_root_noise(np.repeat(eta, G, 0))
                eng.set_forced_playouts(k if full else 0.0)
                eng.set_simulations(budget)
            eng.simulate()
            st = eng.get_states()[0]
            n, q, prior = (a[0] for a in eng.root_stats())
            pi = eng.pruned_policy()[0][0] if prune else eng.policy()[0]
            mv = eng.pick(sample=not (int(st[144]) + 256 * int(st[145]) > thr))
            if full:
                rec = np.zeros(265, np.uint8)
                rec[0] = st[146]
                rec[1:89] = eng.encode()[0]
                rec[93:265] = pi.view(np.uint8)
                rows.append((rec, valid[0], n, q, prior))
            assert (eng.make_moves(mv) == 0).all()
            d += 1; tot["decisions"] += 1; tot["simulations"] += budget - budget % run.threads; tot["samples"] += int(full)
            status = int(eng.status()[0])
            if status != -1:
                break
            assert d < 2000
        z = np.array([outcome_z(status, int(row[0][0])) for row in rows], f32)
        for row, zr in zip(rows, z):
            row[0][89:93] = np.array([zr], f32).view(np.uint8)
        cols = [np.array([row[i] for row in rows], t).reshape(shape) for i, (t, shape) in
                enumerate(((np.uint8, (-1, 265)), (np.uint64, -1), (np.uint32, (-1, 43)), (f32, (-1, 43)), (f32, (-1, 43))))]
        games.append(Game(cols[0], z, *cols[1:]))
    eng.close()
    return games, tot


def assert_streams(records, counters, streams, totals):
    """streams: per game (its expected records, how often the device writes each or None for once).  Every game has records to expect,
    and what is left of them after the repetition lies side by side in the device's bytes; the device wrote that many records and
    nothing else; it counted the retrace's decisions and simulations"""
    blob, total = records.tobytes(), 0
    for g, (want, copies) in enumerate(streams):
        stream = want if copies is None else np.repeat(want, copies, axis=0)
        total += len(stream)
        assert len(want) > 0 and (len(stream) == 0 or stream.tobytes() in blob), f"game {g}: its record stream is not in the device's output"
    assert len(records) == total == counters["samples"], (len(records), total, counters["samples"])
    for key in ("decisions", "simulations"):
        assert counters[key] == totals[key], (key, counters[key], totals[key])


_cache = {}


def cached(kind, run, passes=16, runs=400):
    """kind "retrace": retrace(run); "selfplay": (records, counters) of selfplay(run) played out in runs of `passes` passes"""
    assert kind in ("retrace", "selfplay"), kind
    key = (kind, run._replace(surprise=None, value_mix=None)) if kind == "retrace" else (kind, run, passes, runs)
    if key not in _cache:
        if kind == "retrace":
            _cache[key] = retrace(key[1])
        else:
            eng = selfplay(run)
            _cache[key] = play_out(eng, run.quota, passes, runs)
            eng.close()
    return _cache[key]


def quota_on_slots(slot_counts, configure, sims, base, games=6):
    """a quota of new games on engines of every slot count (two search threads, max_game_rounds 36), configure(eng) before the start:
    the same records (compared sorted bytewise) and the same counts on all of them.  (sorted records, decisions, simulations, samples)"""
    out = []
    for slots in slot_counts:
        eng = engine(2, sims, slots, max_game_rounds=36)
        configure(eng)
        eng.selfplay_start_games(base, games)
        r, c = play_out(eng, games, 64, 4000)
        eng.close()
        assert len(r) == c["samples"]
        out.append((r[np.lexsort(r.T[::-1])], c["decisions"], c["simulations"], c["samples"]))
    for other in out[1:]:
        assert other[0].shape == out[0][0].shape and (other[0] == out[0][0]).all() and other[1:] == out[0][1:]
    assert len(out[0][0]) > 50
    return out[0]
