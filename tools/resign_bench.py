#!/usr/bin/env python3
"""What resignation buys in device self-play (azr_selfplay_set_resign): the same quota of games at the headline configuration (512
games x 100 simulations, T = 2, 20 blocks, bf16, random-init net), first played to the end with resignation off, then with it on;
games/s, decisions per game, records per game (wall clock around the whole quota run, start to the last game's end, ring drained after
every run), the four statistics and the holdout's false-positive share holdout_not_lost / holdout_would_resign.  Without --resign-q the
bound is read off the net: a short quota under the value mix at share 1 writes every decision's root value q into its record, and the
bound is their --quantile.  The lines are also written to --out.

A RANDOM-INIT NET'S NUMBERS DESCRIBE THE MACHINERY, NOT A TUNED THRESHOLD: its root values say nothing about who wins, so the
false-positive share is near that of a coin and the bound is a quantile of noise.  What carries over is the cost of a decision with the
rule on, and how games/s follows the decisions that are not played.  There is no threshold.
    python tools/resign_bench.py [--slots 512] [--games 512] [--mcts 100] [-t 2] [--blocks 20] [--resign-q Q | --quantile 0.25]
                                 [--resign-streak 3] [--resign-holdout 0.1] [--resign-seed 7] [--out profiles/resign_bench.txt]"""
import argparse
import json
import os

import numpy as np

from selfplay_quota import P, common_args, run_quota, warm_up

NOTE = ("# tools/resign_bench.py: a random-init net's numbers describe the machinery (the cost of the rule, games/s against the decisions "
        "not played), not a tuned threshold")


def main():
    ap = argparse.ArgumentParser(parents=[common_args()])
    ap.add_argument("--resign-q", type=float, default=None)
    ap.add_argument("--quantile", type=float, default=0.25)
    ap.add_argument("--probe-games", type=int, default=32)
    ap.add_argument("--resign-streak", type=int, default=3)
    ap.add_argument("--resign-holdout", type=float, default=0.1)
    ap.add_argument("--resign-seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "resign_bench.txt"))
    a = ap.parse_args()
    eng = P.Engine(a.slots, blocks=a.blocks, sims=a.mcts, dtype=P.NET_BF16, threads=a.t)
    eng.init_random(5)
    passes = 4 * (a.mcts + 2)
    lines = [NOTE, "# " + json.dumps({k: v for k, v in vars(a).items() if k != "out"})]
    warm_up(eng, a.slots)
    q_resign = a.resign_q
    if q_resign is None:
        eng.selfplay_set_value_mix(1.0)
        _, _, recs = run_quota(eng, a.probe_games, passes)
        eng.selfplay_set_value_mix(0.0)
        q = np.concatenate(recs)[:, 89:93].copy().view(np.float32)[:, 0]
        q_resign = float(np.quantile(q, a.quantile))
        lines.append(json.dumps(dict(probe_games=a.probe_games, records=len(q), q_min=float(q.min()), q_median=float(np.median(q)),
                                     q_max=float(q.max()), quantile=a.quantile, q_resign=q_resign)))
        print(lines[-1], flush=True)
    rows = []
    for name, streak in (("resignation off", 0), (f"q_resign = {q_resign:.6g}, streak = {a.resign_streak}, holdout = {a.resign_holdout}", a.resign_streak)):
        eng.selfplay_set_resign(q_resign, streak, a.resign_holdout, a.resign_seed)
        dt, c, _ = run_quota(eng, a.games, passes, lambda eng, r: len(r))
        s = eng.selfplay_resign_stats()
        g = max(1, c["games_finished"])
        rows.append(dict(config=name, slots=a.slots, games=c["games_finished"], decisions=c["decisions"], records=c["samples"],
                         simulations=c["simulations"], seconds=round(dt, 3), games_per_s=round(c["games_finished"] / dt, 2),
                         decisions_per_game=round(c["decisions"] / g, 1), records_per_game=round(c["samples"] / g, 1), **s,
                         false_positive_share=round(s["holdout_not_lost"] / s["holdout_would_resign"], 3) if s["holdout_would_resign"] else None))
        lines.append(json.dumps(rows[-1]))
        print(lines[-1], flush=True)
    eng.close()
    off, on = rows
    lines.append(json.dumps(dict(ratio="on / off", games_per_s=round(on["games_per_s"] / off["games_per_s"], 3),
                                 decisions_per_game=round(on["decisions_per_game"] / off["decisions_per_game"], 3),
                                 records_per_game=round(on["records_per_game"] / off["records_per_game"], 3))))
    print(lines[-1], flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
