"""bench.py's launch contract: --gpus N is honoured (N ranks are really started, or the run fails loudly), never
silently ignored.  The CPU half runs here; the GPU half is a 2-rank gloo rehearsal on one card."""
import json
import os
import subprocess
import sys

import pytest

from gpu_common import ROOT

BENCH = os.path.join(ROOT, "bench.py")
# --full for the untimed tail and its record exchange; --no-extra / --no-cpu-baseline keep the rest of --full out
SMALL = ["--games", "32", "--sims", "8", "--blocks", "1", "--steps", "2", "--warmup", "1", "--full", "--no-extra", "--no-cpu-baseline",
         "--tail-seconds", "30"]


def _env(**kw):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    e.update(kw)
    return e


def test_world_size_mismatch_fails_before_anything_runs():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "8"], env=_env(WORLD_SIZE="1", RANK="0"), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1"], env=_env(WORLD_SIZE="2", RANK="0"), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--gpus 1" in r.stderr


def test_gpus_flag_spawns_ranks_and_propagates_their_failure():
    """without a GPU every rank refuses to run (no CPU fallback); the parent must report that, not print a number"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by test_two_rank_bench_on_one_gpu")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2"] + SMALL, env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert "rank exit codes" in r.stderr and "needs an MI355X" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


@pytest.mark.gpu
def test_two_rank_bench_on_one_gpu():
    """plain `python bench.py --gpus 2` (no launcher): two ranks, n_gpus 2, twice the work of one rank, and a record
    exchange that really moved records (gloo backend: both ranks share this box's one card)"""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2"] + SMALL, env=_env(AZR_BENCH_BACKEND="gloo"), capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["value"] > 0
    assert out["config"]["games_per_gpu"] == 32 and "32 concurrent" in out["config"]["workload"]
    ex = out["exchange"]
    assert ex["records_gathered"] > ex["records_this_rank"] > 0 and ex["bytes"] == 265 * ex["records_gathered"]
    assert out["records_dropped"] == 0 and out["errors"] == 0
    one = subprocess.run([sys.executable, BENCH, "--gpus", "1"] + SMALL, env=_env(), capture_output=True, text=True, timeout=900)
    assert one.returncode == 0, one.stderr[-2000:]
    o1 = json.loads([ln for ln in one.stdout.splitlines() if ln.startswith("{")][-1])
    assert o1["n_gpus"] == 1 and o1["exchange"]["records_gathered"] > 0
    assert out["roofline"]["leaf_slots_per_launch"] == o1["roofline"]["leaf_slots_per_launch"] == 64


@pytest.mark.gpu
def test_bench_under_torchrun_as_the_driver_launches_it():
    """the driver's own form for N > 1: python -m torch.distributed.run --nproc-per-node N bench.py --gpus N (gloo here:
    the two ranks share this box's one card)"""
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), BENCH, "--gpus", "2"] + SMALL
    r = subprocess.run(cmd, env=_env(AZR_BENCH_BACKEND="gloo"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1                      # rank 0 prints ONE line
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["exchange"]["records_gathered"] > out["exchange"]["records_this_rank"] > 0
    assert "extra_configs" not in out and "cpu_baseline" not in out      # N > 1: the headline only


def test_help_names_full_and_dump_outputs():
    """--help is answered before torch or HIP is touched: the options a plain run and a --full run are told apart by"""
    r = subprocess.run([sys.executable, BENCH, "--help"], env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_plain_run_times_the_headline_alone_and_dumps_its_outputs(tmp_path):
    """plain `bench.py --gpus 1 --steps K --warmup W`: the headline's result line and nothing that --full adds; --dump-outputs
    writes float32 / float64 arrays under 64 MB, and two runs with the same arguments write the same arrays (games finish inside
    the timed steps, so finished records are among them)"""
    import numpy as np
    args = ["--gpus", "1", "--games", "32", "--sims", "8", "--blocks", "1", "--steps", "500", "--warmup", "1"]
    outs, dumps = [], []
    for i in range(2):
        d = tmp_path / f"run{i}"
        r = subprocess.run([sys.executable, BENCH] + args + ["--dump-outputs", str(d)], env=_env(), capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
        dumps.append({p.name: np.load(p) for p in sorted(d.iterdir())})
    out = outs[0]
    assert out["metric"] == "MCTS simulations/s" and out["unit"] == "simulations/s" and out["higher_is_better"] is True
    assert out["dtype"] == "bf16" and out["value"] > 0 and out["steps"] == 500 and out["warmup"] == 1
    assert abs(out["ms_per_step"] - 1e3 * out["timed_region_s"] / 500) <= 1e-9 * out["ms_per_step"]
    for k in ("extra_configs", "midgame_leg", "cpu_baseline", "config0_play", "optimiser_step", "arena_100", "exchange"):
        assert k not in out, k
    assert out["self_play_games_per_s"] is None and out["games_finished_in_timed_region"] > 0 and out["errors"] == 0
    a, b = dumps
    assert set(a) == set(b) and {"states.npy", "root_visits.npy", "counters.npy", "record_pi.npy"} <= set(a)
    assert all(x.dtype in (np.float32, np.float64) and x.size > 0 for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert a["states.npy"].shape == (32, 160) and a["record_pi.npy"].shape[0] > 0
    assert a["counters.npy"][0] == round(out["value"] * out["timed_region_s"])   # simulations of the timed steps
    for name in a:
        assert a[name].shape == b[name].shape and np.array_equal(a[name], b[name]), name
