"""What the self-play option benches (forced_playouts_bench, playout_cap_bench, surprise_weighting_bench, value_mix_bench) share: the
package, the common arguments, the warm-up and the timed quota run."""
import argparse
import importlib
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
P = importlib.import_module("alphazero-risk_amd")


def common_args():
    """the parent parser of --slots/--games/--mcts/-t/--blocks at the headline configuration"""
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--slots", type=int, default=512)
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--mcts", type=int, default=100)
    ap.add_argument("-t", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=20)
    return ap


def warm_up(eng, slots):
    """first launches, events and staging buffers"""
    eng.selfplay_start_games(1, slots)
    eng.selfplay_run(16)
    eng.discard_samples()


def run_quota(eng, games, passes, on_drain=None):
    """a quota of `games` games played to the end, the ring drained after every run of `passes` passes.  (wall clock of the whole quota
    run, the counters, per drain what on_drain(eng, records) gave, or the records themselves without one)"""
    eng.selfplay_start_games(20260001, games)
    n, out = 0, []
    t0 = time.perf_counter()
    while True:
        eng.selfplay_run(passes)
        c = eng.counters()
        r = eng.drain()
        n += len(r)
        out.append(on_drain(eng, r) if on_drain else r)
        if c["games_finished"] + c["errors"] >= games:
            break
    dt = time.perf_counter() - t0
    assert n == c["samples"] and c["errors"] == 0 and c["records_dropped"] == 0, c
    return dt, c, out
