#!/usr/bin/env python3
"""What policy surprise weighting costs and does in device self-play (azr_selfplay_set_surprise_weighting): the same quota of games
played to the end at the headline configuration (512 games x 100 simulations, T = 2, 20 blocks, bf16, random-init net), twice: weighting
off, then on (--psw-share, --psw-max, --psw-seed).  Per run: games/s, simulations/s (wall clock around the whole quota run, start to
the last game's end, ring drained after every run).  Both runs play the same games and stage the same records — weighting only decides
how often each is written — so the copy count of a record is the number of times the on-run wrote what the off-run wrote once: from
that, records per staged decision, the histogram of copy counts, the share of records left out and the largest count.  (A record the
off-run wrote more than once — two decisions with the same position, policy and outcome — has no copy count of its own and is listed
apart.)  There is no threshold.
    python tools/surprise_weighting_bench.py [--slots 512] [--games 512] [--mcts 100] [-t 2] [--blocks 20] [--psw-share 0.5] [--psw-max 4]"""
import argparse
import json

import numpy as np

from selfplay_quota import P, common_args, run_quota, warm_up


def rows_with_counts(recs):
    """{record bytes: times written}"""
    rows, counts = np.unique(np.ascontiguousarray(recs).view(np.dtype((np.void, recs.shape[1]))).ravel(), return_counts=True)
    return dict(zip((r.tobytes() for r in rows), (int(n) for n in counts)))


def main():
    ap = argparse.ArgumentParser(parents=[common_args()])
    ap.add_argument("--psw-share", type=float, default=0.5)
    ap.add_argument("--psw-max", type=float, default=4.0)
    ap.add_argument("--psw-seed", type=int, default=0)
    a = ap.parse_args()
    eng = P.Engine(a.slots, blocks=a.blocks, sims=a.mcts, dtype=P.NET_BF16, threads=a.t)
    eng.init_random(5)
    warm_up(eng, a.slots)
    rows, written = [], []
    for name, share in (("weighting off", 0.0), (f"share = {a.psw_share}, max = {a.psw_max}", a.psw_share)):
        eng.selfplay_set_surprise_weighting(share, a.psw_max, a.psw_seed)
        dt, c, recs = run_quota(eng, a.games, 4 * (a.mcts + 2))
        written.append(rows_with_counts(np.concatenate(recs)))
        rows.append(dict(config=name, slots=a.slots, games=c["games_finished"], decisions=c["decisions"], records=c["samples"],
                         simulations=c["simulations"], seconds=round(dt, 3), games_per_s=round(c["games_finished"] / dt, 2),
                         simulations_per_s=round(c["simulations"] / dt, 1)))
        print(json.dumps(rows[-1]), flush=True)
    eng.close()
    off, on = rows
    assert (off["games"], off["decisions"], off["simulations"]) == (on["games"], on["decisions"], on["simulations"]), "weighting changed the games"
    assert set(written[1]) <= set(written[0]), "the on-run wrote a record the off-run did not stage"
    single = [b for b, n in written[0].items() if n == 1]
    copies = np.array([written[1].get(b, 0) for b in single])
    hist = np.bincount(copies)
    print(json.dumps(dict(ratio="on / off", games_per_s=round(on["games_per_s"] / off["games_per_s"], 3),
                          simulations_per_s=round(on["simulations_per_s"] / off["simulations_per_s"], 3),
                          records_per_staged_decision=round(on["records"] / off["records"], 4))), flush=True)
    print(json.dumps(dict(staged_records=off["records"], staged_more_than_once=off["records"] - len(single),
                          copy_count_histogram={str(i): int(n) for i, n in enumerate(hist)},
                          share_left_out=round(float((copies == 0).mean()), 4), largest_copy_count=int(copies.max()),
                          mean_copy_count=round(float(copies.mean()), 4))), flush=True)


if __name__ == "__main__":
    main()
