#!/usr/bin/env python3
"""Time the new-vs-old arena of the learn loop (GameGroup::playGames with two AlphaZero players, two networks) on the
device: `games` mirrored games on `slots` engine slots, S simulations per move, THREADS_PER_MCTS T, B blocks, bf16 — or, with
--blocks-b / --dtype-b, an opponent net of another depth and / or arithmetic (random-init nets: a timing, not a strength).
    python tools/arena_bench.py [--games 100] [--slots 128] [--sims 100] [--threads 2] [--blocks 20] [--dtype bf16]
                                [--blocks-b N] [--dtype-b bf16|f16|f32x|f32] [--mcts-b S] [--hp-b C] [--gumbel-m M [--gumbel-tree 1]]
--mcts-b / --hp-b: the opponent player's own simulations per move and PUCT constant (azr_arena_set_opponent_search).
--gumbel-m / --gumbel-tree: both players search by the Gumbel search with sequential halving over M root moves (azr_arena_set_gumbel),
with the improved-policy selection below the root under --gumbel-tree 1; 0 (default) = PUCT, the arena's plain step.
AZR_EXP_LIB=<library>: time that build of the same sources instead (e.g. libazr_hip_test.so with one of its environment hooks)."""
import argparse
import importlib
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
P = importlib.import_module("alphazero-risk_amd")
if os.environ.get("AZR_EXP_LIB"):   # a timing-experiment build of the same sources (never the product library)
    P.binding.lib_path = lambda test_hooks=False: os.environ["AZR_EXP_LIB"]
DTYPES = {"bf16": P.NET_BF16, "f16": P.NET_F16, "f32x": P.NET_F32X, "f32": P.NET_F32}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=100)
    ap.add_argument("--slots", type=int, default=128)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--threads", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--dtype", default="bf16", choices=sorted(DTYPES))
    ap.add_argument("--blocks-b", type=int, default=None, help="residual blocks of the opponent handle's net (default: --blocks)")
    ap.add_argument("--dtype-b", default=None, choices=sorted(DTYPES), help="arithmetic of the opponent handle's net (default: --dtype)")
    ap.add_argument("--mcts-b", type=int, default=None, help="simulations per move of the opponent player (default: --sims)")
    ap.add_argument("--hp-b", type=float, default=None, help="PUCT constant of the opponent player (default: the engine's 1.1)")
    ap.add_argument("--gumbel-m", type=int, default=0, help="root moves of both players' Gumbel search (0 = PUCT)")
    ap.add_argument("--gumbel-tree", type=int, default=0, choices=(0, 1), help="1: the improved-policy selection below the root (needs --gumbel-m)")
    ap.add_argument("--pair-halves", type=int, default=1, help="1: a mirrored pair's two games at the same time on two slots; 0: one after the other on one slot")
    a = ap.parse_args()
    blocks_b = a.blocks if a.blocks_b is None else a.blocks_b
    dtype_b = a.dtype if a.dtype_b is None else a.dtype_b
    kw = {}
    if a.mcts_b is not None and a.mcts_b > a.sims:   # both players' trees live in pools of one size: room for the larger budget
        kw["node_capacity"] = 16 * (a.mcts_b + 1)
    new = P.Engine(a.slots, blocks=a.blocks, sims=a.sims, dtype=DTYPES[a.dtype], threads=a.threads, **kw)
    old = P.Engine(a.slots, blocks=blocks_b, sims=a.sims, dtype=DTYPES[dtype_b], threads=a.threads)
    new.init_random(1)
    old.init_random(2)
    new.arena_set_opponent(old)
    budget = ""
    if a.mcts_b is not None or a.hp_b is not None:
        new.arena_set_opponent_search(a.mcts_b, a.hp_b)
        budget = f" (S={a.sims if a.mcts_b is None else a.mcts_b} hp={1.1 if a.hp_b is None else a.hp_b})"
    if a.gumbel_m > 0:
        for player in (P.PLAYER_ALPHAZERO, P.PLAYER_ALPHAZERO_B):
            new.arena_set_gumbel(player, a.gumbel_m, tree=a.gumbel_tree)
        budget += f" Gumbel m={a.gumbel_m}" + (" tree" if a.gumbel_tree else "")
    new.arena_start(P.PLAYER_ALPHAZERO, P.PLAYER_ALPHAZERO_B, a.games, 0, P.MIRROR_CONCURRENT if a.pair_halves else P.MIRROR_SEQUENTIAL, 20260001)
    t0 = time.time()
    while not new.arena_run(256):
        pass
    dt = time.time() - t0
    r = new.arena_results()
    print(f"{a.games} games on {a.slots} slots, S={a.sims} T={a.threads} {a.dtype} B={a.blocks} vs {dtype_b} B={blocks_b}{budget}: {dt:.2f} s, results {r}, "
          f"tower_fallbacks {new.counters()['tower_fallbacks']}", flush=True)


if __name__ == "__main__":
    main()
