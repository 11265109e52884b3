#!/usr/bin/env python3
"""What the value mix costs and does in device self-play (azr_selfplay_set_value_mix): the same quota of games played to the end at the
headline configuration (512 games x 100 simulations, T = 2, 20 blocks, bf16, random-init net), with the mix off and on (--q-share),
alternating, --repeats times each.  Per run: games/s, simulations/s (wall clock around the whole quota run, start to the last game's
end, ring drained after every run) and the tree step's average launch in ms (azr_profile_last_run, averaged over the run's launches).
Both configurations play the same games and write the same records but for the four value bytes, so the records pair up: from that the
mean |z' - z|, a histogram of z', and the share of records whose root value q disagrees in sign with the outcome z (q is recovered
from the pair as (z' - (1 - share) z) / share, up to rounding; a drawn game's records, z = 0, are counted apart).  There is no threshold.
    python tools/value_mix_bench.py [--slots 512] [--games 512] [--mcts 100] [-t 2] [--blocks 20] [--q-share 0.5] [--repeats 2]"""
import argparse
import json

import numpy as np

from selfplay_quota import P, common_args, run_quota, warm_up


def main():
    ap = argparse.ArgumentParser(parents=[common_args()])
    ap.add_argument("--q-share", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=2)
    a = ap.parse_args()
    eng = P.Engine(a.slots, blocks=a.blocks, sims=a.mcts, dtype=P.NET_BF16, threads=a.t)
    eng.init_random(5)
    warm_up(eng, a.slots)
    rows, recs = {"off": [], "on": []}, {}
    for rep in range(a.repeats):
        for name, share in (("off", 0.0), ("on", a.q_share)):
            eng.selfplay_set_value_mix(share)
            dt, c, drains = run_quota(eng, a.games, 4 * (a.mcts + 2), lambda eng, r: (r, eng.profile_last_run()))
            recs[name] = np.concatenate([r for r, _ in drains])
            tree_ms = sum(p["tree_ms"] * p["launches"] for _, p in drains) / max(sum(p["launches"] for _, p in drains), 1)
            rows[name].append(dict(config="mix " + name + ("" if name == "off" else f", q_share = {a.q_share}"), run=rep + 1, slots=a.slots,
                                   games=c["games_finished"], decisions=c["decisions"], records=c["samples"], simulations=c["simulations"],
                                   seconds=round(dt, 3), games_per_s=round(c["games_finished"] / dt, 2),
                                   simulations_per_s=round(c["simulations"] / dt, 1), tree_step_ms=round(tree_ms, 5)))
            print(json.dumps(rows[name][-1]), flush=True)
    eng.close()
    keys = ("games", "decisions", "records", "simulations")
    assert len({tuple(r[k] for k in keys) for rs in rows.values() for r in rs}) == 1, "the mix changed the games"
    med = {n: {k: float(np.median([r[k] for r in rs])) for k in ("games_per_s", "simulations_per_s", "tree_step_ms", "seconds")} for n, rs in rows.items()}
    print(json.dumps(dict(median=med, ratio_on_off={k: round(med["on"][k] / med["off"][k], 4) for k in med["on"]})), flush=True)
    # pair the records up: equal outside the value bytes
    mask = np.ones(265, bool); mask[89:93] = False
    off, on = (r[np.lexsort(r[:, mask].T[::-1])] for r in (recs["off"], recs["on"]))
    assert (off[:, mask] == on[:, mask]).all(), "the mix changed more than the value bytes"
    z = off[:, 89:93].copy().view(np.float32)[:, 0].astype(np.float64)
    zz = on[:, 89:93].copy().view(np.float32)[:, 0].astype(np.float64)
    assert set(z.tolist()) <= {-1.0, 0.0, 1.0} and (np.abs(zz) <= 1).all()
    s = float(np.float32(a.q_share))
    q = (zz - (1.0 - s) * z) / s
    decided = z != 0
    edges = np.linspace(-1, 1, 11)
    hist = np.histogram(zz, edges)[0]
    print(json.dumps(dict(records=len(z), decided=int(decided.sum()), drawn=int((~decided).sum()),
                          mean_abs_dz=round(float(np.abs(zz - z).mean()), 4),
                          mean_abs_dz_decided=round(float(np.abs(zz - z)[decided].mean()), 4) if decided.any() else None,
                          q_z_sign_disagree_share_of_decided=round(float((q * z < 0)[decided].mean()), 4) if decided.any() else None,
                          mean_q_times_z_decided=round(float((q * z)[decided].mean()), 4) if decided.any() else None,
                          z_mix_histogram={"[%.1f, %.1f%s" % (edges[i], edges[i + 1], "]" if i == 9 else ")"): int(n) for i, n in enumerate(hist)})),
          flush=True)


if __name__ == "__main__":
    main()
