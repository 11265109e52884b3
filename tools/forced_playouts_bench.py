#!/usr/bin/env python3
"""What forced playouts and policy target pruning cost and change in device self-play (azr_selfplay_set_forced_playouts): the same
quota of games played to the end at the headline configuration (512 games x 100 simulations, T = 2, 20 blocks, bf16, random-init
net) with Dirichlet(--dir-alpha) root noise, three times: forcing off, forcing on (--forced-k), forcing on with pruning.  Per run:
games/s, simulations/s (wall clock around the whole quota run, start to the last game's end, ring drained after every run) and the
mean number of non-zero pi entries per written record.  Forcing changes the games, so the three runs do not play the same moves;
the two forced runs do (pruning only rewrites pi), so their game and simulation counts agree.  There is no threshold.
    python tools/forced_playouts_bench.py [--slots 512] [--games 512] [--mcts 100] [-t 2] [--blocks 20] [--dir-alpha 0.3] [--forced-k 2]"""
import argparse
import json

import numpy as np

from selfplay_quota import P, common_args, run_quota, warm_up


def main():
    ap = argparse.ArgumentParser(parents=[common_args()])
    ap.add_argument("--dir-alpha", type=float, default=0.3)
    ap.add_argument("--dir-seed", type=int, default=7)
    ap.add_argument("--forced-k", type=float, default=2.0)
    a = ap.parse_args()
    eng = P.Engine(a.slots, blocks=a.blocks, sims=a.mcts, dtype=P.NET_BF16, threads=a.t)
    eng.init_random(5)
    eng.selfplay_set_dirichlet(a.dir_alpha, a.dir_seed)
    rows = []
    warm_up(eng, a.slots)
    for name, k, prune in (("forcing off", 0.0, False), (f"k = {a.forced_k}", a.forced_k, False), (f"k = {a.forced_k}, pruned target", a.forced_k, True)):
        eng.selfplay_set_forced_playouts(k, prune)
        dt, c, nonzero = run_quota(eng, a.games, 4 * (a.mcts + 2), lambda eng, r: int((np.ascontiguousarray(r[:, 93:265]).view(np.float32) != 0).sum()))
        nz = sum(nonzero) / max(c["samples"], 1)
        rows.append(dict(config=name, slots=a.slots, games=c["games_finished"], decisions=c["decisions"], records=c["samples"],
                         simulations=c["simulations"], seconds=round(dt, 3), games_per_s=round(c["games_finished"] / dt, 2),
                         simulations_per_s=round(c["simulations"] / dt, 1), nonzero_pi_per_record=round(nz, 2)))
        print(json.dumps(rows[-1]), flush=True)
    off = rows[0]
    for on in rows[1:]:
        print(json.dumps(dict(ratio=on["config"] + " / off", games_per_s=round(on["games_per_s"] / off["games_per_s"], 3),
                              simulations_per_s=round(on["simulations_per_s"] / off["simulations_per_s"], 3),
                              nonzero_pi_per_record=round(on["nonzero_pi_per_record"] / off["nonzero_pi_per_record"], 3))), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
