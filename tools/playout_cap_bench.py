#!/usr/bin/env python3
"""What playout cap randomisation buys in device self-play (azr_selfplay_set_playout_cap): the same quota of games played to the
end at the headline configuration (512 games x 100 simulations, T = 2, 20 blocks, bf16, random-init net), first with the cap off,
then with full_prob P and fast budget N; games/s, decisions/s, records/s and simulations/s of each, wall clock around the whole quota
run (start to the last game's end, ring drained after every run).  The only arithmetic expectation printed beside them is the
ceiling: a decision costs S descents without the cap and P*S + (1-P)*F on average with it, so decisions/s can rise by at most
S / (P*S + (1-P)*F).  There is no threshold.
    python tools/playout_cap_bench.py [--slots 512] [--games 512] [--mcts 100] [-t 2] [--blocks 20] [--cap-prob 0.25] [--cap-fast 20]"""
import argparse
import json

from selfplay_quota import P, common_args, run_quota, warm_up


def main():
    ap = argparse.ArgumentParser(parents=[common_args()])
    ap.add_argument("--cap-prob", type=float, default=0.25)
    ap.add_argument("--cap-fast", type=int, default=20)
    ap.add_argument("--cap-seed", type=int, default=7)
    a = ap.parse_args()
    eng = P.Engine(a.slots, blocks=a.blocks, sims=a.mcts, dtype=P.NET_BF16, threads=a.t)
    eng.init_random(5)
    S, F = a.mcts - a.mcts % a.t, a.cap_fast - a.cap_fast % a.t
    rows = []
    warm_up(eng, a.slots)
    for name, prob, fast in (("cap off", 1.0, 0), (f"P = {a.cap_prob}, N = {a.cap_fast}", a.cap_prob, a.cap_fast)):
        eng.selfplay_set_playout_cap(prob, fast, a.cap_seed)
        dt, c, _ = run_quota(eng, a.games, 4 * (a.mcts + 2), lambda eng, r: len(r))
        rows.append(dict(config=name, slots=a.slots, games=c["games_finished"], decisions=c["decisions"], records=c["samples"],
                         simulations=c["simulations"], seconds=round(dt, 3), games_per_s=round(c["games_finished"] / dt, 2),
                         decisions_per_s=round(c["decisions"] / dt, 1), records_per_s=round(c["samples"] / dt, 1),
                         simulations_per_s=round(c["simulations"] / dt, 1)))
        print(json.dumps(rows[-1]), flush=True)
    off, on = rows
    print(json.dumps(dict(ratio="capped / off", games_per_s=round(on["games_per_s"] / off["games_per_s"], 3),
                          decisions_per_s=round(on["decisions_per_s"] / off["decisions_per_s"], 3),
                          records_per_s=round(on["records_per_s"] / off["records_per_s"], 3),
                          simulations_per_s=round(on["simulations_per_s"] / off["simulations_per_s"], 3),
                          decisions_per_s_ceiling=round(S / (a.cap_prob * S + (1 - a.cap_prob) * F), 3))), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
