#!/usr/bin/env python3
"""Time train-data's generation step on the device (trainOnGeneratedData, alphazero_trainer.cpp:236-275): Script-vs-Script
and Script-vs-Random games with scripted collection on, the ring drained after every run; games/s and records/s per slot
count, the best of `--reps` timed runs after one warm-up.  `--off` times the same arenas without recording.
    python tools/scripted_data_bench.py [--slots 256,1024,4096] [--games-per-slot 10] [--reps 3] [--off]"""
import argparse
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
P = importlib.import_module("alphazero-risk_amd")


def run(eng, k0, k1, games, record):
    eng.arena_collect_scripted_samples(record)
    eng.arena_start(k0, k1, games, 0, P.MIRROR_SEQUENTIAL, 20260001)
    t0 = time.perf_counter()
    n, runs = 0, 0
    while True:
        fin = eng.arena_run(2)
        runs += 1
        if record:
            n += len(eng.drain())
        if fin:
            break
    dt = time.perf_counter() - t0
    return dt, n, runs, eng.arena_results()["count"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="256,1024,4096")
    ap.add_argument("--games-per-slot", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--off", action="store_true", help="scripted collection off (the arena alone)")
    a = ap.parse_args()
    for G in (int(x) for x in a.slots.split(",")):
        eng = P.Engine(G, blocks=1, sims=1, dtype=P.NET_F32, node_capacity=64, sample_capacity=2048)
        for name, k1 in (("script-vs-script", P.PLAYER_SCRIPT), ("script-vs-random", P.PLAYER_RANDOM)):
            games = G * a.games_per_slot
            run(eng, P.PLAYER_SCRIPT, k1, games, not a.off)   # warm-up
            best = min((run(eng, P.PLAYER_SCRIPT, k1, games, not a.off) for _ in range(a.reps)), key=lambda r: r[0])
            dt, n, runs, played = best
            print(json.dumps(dict(pairing=name, slots=G, games=played, records=n, runs=runs, seconds=round(dt, 4),
                                  games_per_s=round(played / dt, 1), records_per_s=round(n / dt, 1), recording=not a.off)),
                  flush=True)
        eng.close()


if __name__ == "__main__":
    main()
