#!/usr/bin/env python3
"""What the Gumbel root search costs and what it writes in device self-play (azr_selfplay_set_gumbel): the same quota of games with it
off, on, and on with the improved-policy selection below the root (azr_selfplay_set_gumbel_tree; the arm "on + tree") at --mcts 16 and
100 (T = 2, 20 blocks, bf16, random-init net), --repeat runs each, alternating off, on, on + tree, off, ...;
games/s and simulations/s (wall clock around the whole quota run, ring drained after every run), the tree step's average launch
(azr_profile_last_run, averaged over the quota's runs) and the mean entropy of the recorded pi in nats.  The lines are also written to
--out.

A RANDOM-INIT NET'S NUMBERS DESCRIBE THE MACHINERY: what the root-level selection, the selection below the root and the decision cost
per tree step, and how flat the recorded target is.  Whether the target trains a stronger net is not measured here.  There is no threshold.
    python tools/gumbel_bench.py [--slots 512] [--games 512] [-t 2] [--blocks 20] [--budgets 16,100] [--gumbel-m 16] [--gumbel-cvisit 50]
                                 [--gumbel-cscale 0.5] [--gumbel-seed 7] [--repeat 3] [--out profiles/gumbel_bench.txt]"""
import argparse
import json
import os

import numpy as np

from selfplay_quota import P, common_args, run_quota, warm_up

NOTE = "# tools/gumbel_bench.py: a random-init net's numbers describe the machinery (the cost per tree step, the flatness of the target), not playing strength"


def entropy_sum(eng, recs):
    """(sum of the records' entropies in nats, records, the tree step's average launch of the run before this drain)"""
    pi = recs[:, 93:265].copy().view(np.float32).astype(np.float64)
    h = -(pi * np.log(np.where(pi > 0, pi, 1.0))).sum()
    return float(h), len(recs), eng.profile_last_run()["tree_ms"]


def main():
    ap = argparse.ArgumentParser(parents=[common_args()])
    ap.add_argument("--budgets", default="16,100")
    ap.add_argument("--gumbel-m", type=int, default=16)
    ap.add_argument("--gumbel-cvisit", type=float, default=50.0)
    ap.add_argument("--gumbel-cscale", type=float, default=0.5)
    ap.add_argument("--gumbel-seed", type=int, default=7)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "gumbel_bench.txt"))
    a = ap.parse_args()
    lines = [NOTE, "# " + json.dumps({k: v for k, v in vars(a).items() if k not in ("out", "mcts")})]
    for mcts in (int(b) for b in a.budgets.split(",")):
        eng = P.Engine(a.slots, blocks=a.blocks, sims=mcts, dtype=P.NET_BF16, threads=a.t)
        eng.init_random(5)
        passes = 4 * (mcts + 2)
        warm_up(eng, a.slots)
        rows = {"off": [], "on": [], "on + tree": []}
        for rep in range(a.repeat):
            for name, m, tree in (("off", 0, 0), ("on", a.gumbel_m, 0), ("on + tree", a.gumbel_m, 1)):
                eng.selfplay_set_gumbel(m, a.gumbel_cvisit, a.gumbel_cscale, a.gumbel_seed)
                eng.selfplay_set_gumbel_tree(tree)
                dt, c, out = run_quota(eng, a.games, passes, entropy_sum)
                n = max(1, sum(o[1] for o in out))
                rows[name].append(dict(mcts=mcts, gumbel=name, m=m, run=rep, games=c["games_finished"], decisions=c["decisions"], records=c["samples"],
                                       simulations=c["simulations"], seconds=round(dt, 3), games_per_s=round(c["games_finished"] / dt, 2),
                                       simulations_per_s=round(c["simulations"] / dt), tree_step_ms=round(float(np.mean([o[2] for o in out])), 5),
                                       mean_pi_entropy=round(sum(o[0] for o in out) / n, 6)))
                lines.append(json.dumps(rows[name][-1]))
                print(lines[-1], flush=True)
        eng.close()
        med = {k: {f: float(np.median([r[f] for r in v])) for f in ("games_per_s", "simulations_per_s", "tree_step_ms", "mean_pi_entropy")} for k, v in rows.items()}
        lines.append(json.dumps(dict(mcts=mcts, medians=med, on_over_off={f: round(med["on"][f] / med["off"][f], 3) for f in med["on"]},
                                     tree_over_on={f: round(med["on + tree"][f] / med["on"][f], 3) for f in med["on"]})))
        print(lines[-1], flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
