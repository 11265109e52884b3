#!/usr/bin/env python3
"""How much of a net's strength is search?  One net on both sides of a two-net arena — one checkpoint, or random weights — player A at
--mcts-a simulations per move, player B at each budget of --mcts-b in turn (azr_arena_set_opponent_search), `--games` games in
mirrored pairs per rung.  Prints per rung B's share of the decided games with its 95 % Wilson interval and the wall time: the
win share against simulation count of the AlphaZero papers.  --blocks-b / --dtype-b give B another depth or arithmetic, which puts
"how many simulations make up for 15 blocks" and "is bf16 at 3 x the simulations stronger than f32x" on the same axis.
    python tools/search_ladder.py [--checkpoint FILE [--checkpoint-b FILE] | --seed N] [--mcts-a 32] [--mcts-b 2,4,8,16,32,64,128]
                                  [--hp-a 1.1] [--hp-b 1.1] [--blocks 20] [--dtype bf16] [--blocks-b N] [--dtype-b bf16|f16|f32x|f32]
                                  [--games 100] [--threads 2] [--slots 128] [--base-seed 20260001]
                                  [--gumbel-m-a M] [--gumbel-m-b M] [--gumbel-tree-a 1] [--gumbel-tree-b 1] [--gumbel-cvisit 50] [--gumbel-cscale 0.5]
--gumbel-m-a / --gumbel-m-b give a side the Gumbel search with sequential halving over M root moves in place of PUCT (azr_arena_set_gumbel;
deterministic), --gumbel-tree-a / -b its improved-policy selection below the root: PUCT against Gumbel at one net and equal budgets is
`--mcts-a 16 --mcts-b 16 --gumbel-m-b 16`.
A checkpoint holds one depth: with --blocks-b other than --blocks name B's own (--checkpoint-b).  Without a checkpoint the nets are
random-init from --seed; such a net knows nothing about the game, so the table then shows the tool, not a strength."""
import argparse
import importlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from precision_arena import DTYPES, wilson  # noqa: E402

P = importlib.import_module("alphazero-risk_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--checkpoint-b", default=None, help="B's checkpoint when --blocks-b differs from --blocks")
    ap.add_argument("--seed", type=int, default=20260002, help="random-init seed when no --checkpoint is given")
    ap.add_argument("--mcts-a", type=int, default=32)
    ap.add_argument("--mcts-b", default="2,4,8,16,32,64,128", help="B's budgets, one rung each")
    ap.add_argument("--hp-a", type=float, default=1.1)
    ap.add_argument("--hp-b", type=float, default=None, help="B's PUCT constant (default: --hp-a)")
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--dtype", default="bf16", choices=sorted(DTYPES))
    ap.add_argument("--blocks-b", type=int, default=None)
    ap.add_argument("--dtype-b", default=None, choices=sorted(DTYPES))
    ap.add_argument("--games", type=int, default=100)
    ap.add_argument("--threads", type=int, default=2)
    ap.add_argument("--slots", type=int, default=128)
    ap.add_argument("--base-seed", type=int, default=20260001)
    ap.add_argument("--gumbel-m-a", type=int, default=0, help="root moves of A's Gumbel search (0 = PUCT)")
    ap.add_argument("--gumbel-m-b", type=int, default=0, help="root moves of B's Gumbel search (0 = PUCT)")
    ap.add_argument("--gumbel-tree-a", type=int, default=0, choices=(0, 1), help="1: A selects below the root by the improved policy (needs --gumbel-m-a)")
    ap.add_argument("--gumbel-tree-b", type=int, default=0, choices=(0, 1), help="1: B selects below the root by the improved policy (needs --gumbel-m-b)")
    ap.add_argument("--gumbel-cvisit", type=float, default=50.0)
    ap.add_argument("--gumbel-cscale", type=float, default=0.5)
    a = ap.parse_args()
    rungs = [int(x) for x in a.mcts_b.split(",") if x]
    blocks_b = a.blocks if a.blocks_b is None else a.blocks_b
    dtype_b = a.dtype if a.dtype_b is None else a.dtype_b
    if a.checkpoint and blocks_b != a.blocks and not a.checkpoint_b:
        ap.error("--blocks-b differs from --blocks: a checkpoint holds one depth, name B's with --checkpoint-b")
    # both players' trees live in node pools of one size: room for the largest budget on the ladder
    cap = 16 * (max(rungs + [a.mcts_a]) + 1)
    ea = P.Engine(a.slots, blocks=a.blocks, sims=a.mcts_a, dtype=DTYPES[a.dtype], threads=a.threads, hp_exploration=a.hp_a, node_capacity=cap)
    eb = P.Engine(a.slots, blocks=blocks_b, sims=a.mcts_a, dtype=DTYPES[dtype_b], threads=a.threads)
    if a.checkpoint:
        ea.load(a.checkpoint)
        eb.load(a.checkpoint_b or a.checkpoint)
    else:
        ea.init_random(a.seed)
        if blocks_b == a.blocks:
            eb.set_weights(ea.get_weights())   # the same fp32 parameter vector; each handle packs it for its own arithmetic
        else:
            eb.init_random(a.seed)
    ea.arena_set_opponent(eb)
    ea.arena_set_gumbel(P.PLAYER_ALPHAZERO, a.gumbel_m_a, a.gumbel_cvisit, a.gumbel_cscale, a.gumbel_tree_a)
    ea.arena_set_gumbel(P.PLAYER_ALPHAZERO_B, a.gumbel_m_b, a.gumbel_cvisit, a.gumbel_cscale, a.gumbel_tree_b)
    search = lambda m, tree: f"Gumbel m {m}" + (" (tree)" if tree else "") + f" c_visit {a.gumbel_cvisit:g} c_scale {a.gumbel_cscale:g}" if m > 0 else "PUCT"   # noqa: E731
    what = f"checkpoint {a.checkpoint}" if a.checkpoint else f"random-init seed {a.seed}"
    print(f"A = {a.dtype} {a.blocks} blocks at {a.mcts_a} simulations, hp {a.hp_a}, {search(a.gumbel_m_a, a.gumbel_tree_a)}; B = {dtype_b} {blocks_b} blocks, hp "
          f"{a.hp_a if a.hp_b is None else a.hp_b}, {search(a.gumbel_m_b, a.gumbel_tree_b)}; {what}, T = {a.threads}, {a.games} games per rung on {a.slots} slots")
    print(f"{'B sims':>7} {'count':>6} {'draw':>5} {'A wins':>7} {'B wins':>7} {'B share':>8}  95 % Wilson      wall s   dropped")
    for s in rungs:
        ea.arena_set_opponent_search(s, a.hp_b)
        ea.arena_start(P.PLAYER_ALPHAZERO, P.PLAYER_ALPHAZERO_B, a.games, 0, P.MIRROR_CONCURRENT, a.base_seed)
        t0 = time.time()
        while not ea.arena_run(256):
            pass
        dt = time.time() - t0
        r = ea.arena_results()
        c = ea.counters()
        wa, wb = r["win"]
        lo, hi = wilson(wb, wa + wb)
        share = wb / (wa + wb) if wa + wb else float("nan")
        print(f"{s - s % a.threads:>7} {r['count']:>6} {r['draw']:>5} {wa:>7} {wb:>7} {share:>8.3f}  [{lo:.3f}, {hi:.3f}] {dt:>8.2f} "
              f"{c['nodes_dropped'] + c['errors']:>9}", flush=True)
    ea.arena_set_opponent(None)
    ea.close(); eb.close()


if __name__ == "__main__":
    main()
