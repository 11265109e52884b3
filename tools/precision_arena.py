#!/usr/bin/env python3
"""Does a cheaper net arithmetic cost games?  The SAME weights on both handles of a two-net arena, one evaluated in --dtype-a
and the other in --dtype-b (bf16 | f16 | f32x | f32), `--games` games in mirrored pairs (both players start every deal once).
Prints the GameResults line and a 95 % Wilson score interval of A's share of the decided games.
    python tools/precision_arena.py [--checkpoint FILE | --seed N] [--dtype-a bf16] [--dtype-b f32x] [--blocks 20] [--games 1000]
                                    [--mcts 100] [--threads 2] [--slots 128] [--base-seed 20260001]
--checkpoint: an AZRW file (azr_nn_save; its depth must be --blocks).  Without one the nets are random-init from --seed: such a net
knows nothing about the game, so its result says whether the two arithmetics play DIFFERENT games, not which one is stronger."""
import argparse
import importlib
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
P = importlib.import_module("alphazero-risk_amd")
DTYPES = {"bf16": P.NET_BF16, "f16": P.NET_F16, "f32x": P.NET_F32X, "f32": P.NET_F32}


def wilson(k, n, z=1.959964):
    """Wilson score interval of a binomial share k / n (Wilson 1927)"""
    if n == 0:
        return 0.0, 1.0
    p = k / n
    d = 1 + z * z / n
    c = (p + z * z / (2 * n)) / d
    w = z * math.sqrt(p * (1 - p) / n + z * z / (4 * n * n)) / d
    return max(0.0, c - w), min(1.0, c + w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--seed", type=int, default=20260002, help="random-init seed when no --checkpoint is given")
    ap.add_argument("--dtype-a", default="bf16", choices=sorted(DTYPES))
    ap.add_argument("--dtype-b", default="f32x", choices=sorted(DTYPES))
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--games", type=int, default=1000)
    ap.add_argument("--mcts", type=int, default=100)
    ap.add_argument("--threads", type=int, default=2)
    ap.add_argument("--slots", type=int, default=128)
    ap.add_argument("--base-seed", type=int, default=20260001)
    a = ap.parse_args()
    ea = P.Engine(a.slots, blocks=a.blocks, sims=a.mcts, dtype=DTYPES[a.dtype_a], threads=a.threads)
    eb = P.Engine(a.slots, blocks=a.blocks, sims=a.mcts, dtype=DTYPES[a.dtype_b], threads=a.threads)
    if a.checkpoint:
        ea.load(a.checkpoint)
    else:
        ea.init_random(a.seed)
    eb.set_weights(ea.get_weights())   # the same fp32 parameter vector; each handle packs it for its own arithmetic
    ea.arena_set_opponent(eb)
    ea.arena_start(P.PLAYER_ALPHAZERO, P.PLAYER_ALPHAZERO_B, a.games, 0, P.MIRROR_CONCURRENT, a.base_seed)
    t0 = time.time()
    while not ea.arena_run(256):
        pass
    dt = time.time() - t0
    r = ea.arena_results()
    c = ea.counters()
    ea.arena_set_opponent(None)
    ea.close(); eb.close()
    wa, wb = r["win"]
    lo, hi = wilson(wa, wa + wb)
    what = f"checkpoint {a.checkpoint}" if a.checkpoint else f"random-init seed {a.seed}"
    print(f"A = {a.dtype_a}, B = {a.dtype_b}, {what}, {a.blocks} blocks, {a.mcts} simulations, T = {a.threads}: {dt:.1f} s")
    print(f"GameResults: count {r['count']} draw {r['draw']} | A wins {wa} (started {r['win_and_started'][0]}) | "
          f"B wins {wb} (started {r['win_and_started'][1]}) | errors {c['errors']} nodes_dropped {c['nodes_dropped']}")
    share = wa / (wa + wb) if wa + wb else float("nan")
    print(f"A's share of the {wa + wb} decided games: {share:.3f}, 95 % Wilson interval [{lo:.3f}, {hi:.3f}]"
          + ("  (0.5 is inside: no difference shown)" if lo <= 0.5 <= hi else "  (0.5 is outside)"))


if __name__ == "__main__":
    main()
