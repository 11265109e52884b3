"""GPU: BASELINE configs[3] / configs[4] rehearsed at their real rank counts and shapes on the ONE MI355X of a gpurun box.

A box allows at most 6 processes on its card (the test runner is one of them), so:
  * the data-parallel optimiser step at WORLD 8 and the reference's BATCH_SIZE 512 (64-record shares -> the small-batch conv kernel
    t_conv_q, 8-board weight-gradient slices) runs as 8 engine handles driven by 8 host threads of THIS process, the sums meeting in an
    in-process all-reduce (tests/dp_group.py: rank order, so the ranks must end bit-equal) — the C-ABI's "one handle = one host thread" contract at 8
    handles on one device is exactly what the C++ host's one-thread-per-GPU structure relies on;
  * the multi-PROCESS paths run over gloo with the ranks sharing the card, at the largest world that fits beside the runner: bench.py's
    own rank spawner (its parent never touches HIP) + record gather with 5 ranks, one learn.py iteration under torchrun (whose agent
    process opens the GPU too) with 4 — ragged game / pair / record counts in both;
  * the C++ host CLI's in-process multi-GPU path (one host thread per GPU, temp.bin weight hand-over, split arena, merged results)
    runs with --gpus 2 and both logical GPUs mapped onto device 0 (--devices 0,0).
Reference structures replaced: one self-play thread per GPU + vector concat (alphazero_trainer.cpp:41-62), GPU-0-trains + temp.bin
(alphazero_gpu_cluster.cpp:144-164,221-231), GameGroup's thread-per-pair fan-out (game.cpp:277-312)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import azr_testlib as T
import dp_group as DG
import train_replay as TR
from gpu_common import ROOT, pkg

pytestmark = pytest.mark.gpu
HOST = os.path.join(ROOT, "alphazero-risk_amd", "host")
EXE = os.path.join(HOST, "AlphaZero_Risk_hip")


def _port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _env(**kw):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    e.update(HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"), **kw)
    return e


def _records(n, seed):
    rng = np.random.default_rng(seed)
    in88 = np.load(os.path.join(T.GOLDEN, "encode.npz"))["in88"]
    rec = np.zeros((n, 265), np.uint8)
    rec[:, 0] = rng.integers(0, 2, n)
    rec[:, 1:89] = in88[rng.integers(0, len(in88), n)]
    rec[:, 89:93] = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), n).view(np.uint8).reshape(n, 4)
    pi = rng.random((n, 43)).astype(np.float32) ** 3
    pi /= pi.sum(1, keepdims=True)
    rec[:, 93:265] = pi.view(np.uint8).reshape(n, 172)
    return rec


def _rel_l2_worst(blocks, g, g1):
    """the measure of tests/test_gpu_train.py's batch-512 case: the worst relative L2 difference per tensor (gamma / beta of a batch norm)"""
    worst = 0.0
    for name, off, n in T.net_layout(blocks):
        a, b = g[off:off + n].astype(np.float64), g1[off:off + n].astype(np.float64)
        if name.endswith("_bn"):
            a, b = a[:n // 2], b[:n // 2]
        nb = np.linalg.norm(b)
        if nb > 0:
            worst = max(worst, np.linalg.norm(a - b) / nb)
    return worst


def test_world8_batch512_data_parallel_step_in_one_process():
    """configs[4]'s optimiser step at its real shape: 8 ranks, BATCH_SIZE 512 (settings.h:74) -> 64-record shares, 20-block layout
    rules at B = 2, two steps on a tests/dp_group.py::DpGroup.  At BOTH steps: ranks bit-equal, the all-reduce count; the step equals
    bit for bit the step of a fresh group given the weights from before it (a step is a function of weights and minibatch — the Adam
    state the second step carries is restated on the host, TR.adam_trajectory); losses and gradients against the single-GPU engine
    started from those same weights: losses 2e-5, relative L2 per tensor 3e-3, and the |dw| statistics between the group's weights and
    Adam (on the moments the group's own gradients left) on the single-GPU gradients.
    Measured, not asserted (profiles/train_dp_measured.txt): how much of the gradient difference that a single-GPU TRAJECTORY shows at
    its second step against the group's (7e-3 .. 1.2e-2 relative L2) the difference of the two weight vectors alone reproduces."""
    P = pkg()
    world, bs, blocks = 8, 512, 2
    flat = T.make_net_flat(blocks, seed=9, perturb_bn=True)
    rec = _records(2 * bs, seed=5)
    k = TR.kinds(blocks)
    tr = k > 0
    lay = TR.train.layout(blocks)[0]

    def engine():
        return P.Engine(4, blocks=blocks, sims=1, dtype=P.NET_F32, node_capacity=64)

    def single_step(w, mb):
        """(losses, gradients, weights behind the step) of a fresh single-GPU engine given the weights w"""
        e = engine()
        e.set_weights(w)
        out = (e.train_batch(mb), e.train_grads(), e.get_weights())
        e.close()
        return out

    group = DG.DpGroup(world, engine)
    group.set_weights(flat)
    ref = engine()            # the single-GPU TRAJECTORY: one engine through both minibatches
    ref.set_weights(flat)
    per_step = 2 * (2 * blocks + 1 + 1) + 2
    m, v = np.zeros_like(flat), np.zeros_like(flat)
    trace = []
    for step in range(2):
        mb = rec[step * bs:(step + 1) * bs]
        w0 = group.get_weights()                       # (asserts the ranks bit-equal)
        loss = group.train_batch(mb)                   # (asserts equal losses on all ranks and the shuffle stream consumed)
        g, w1 = group.train_grads(), group.get_weights()
        DG.assert_calls(group, step + 1, per_step, len(flat))
        fresh_state = not trace                        # no step has run on the group yet: m = v = 0, as on a fresh engine
        trace.append(TR.Step("train", bs, w0, mb, tuple(loss), g, w1, fresh_state))
        # ---- the same step on a fresh group from the weights in front of it: bit for bit
        fresh = DG.DpGroup(world, engine)
        fresh.set_weights(w0)
        loss_f = fresh.train_batch(mb)
        g_f, w1_f = fresh.train_grads(), fresh.get_weights()
        fresh.close()
        assert tuple(loss) == tuple(loss_f), (step, loss, loss_f)
        assert TR.first_difference(g, g_f, lay) is None, (step, TR.first_difference(g, g_f, lay))
        assert TR.first_difference(np.where(tr, 0, w1), np.where(tr, 0, w1_f), lay) is None, step    # moving statistics
        if fresh_state:
            assert TR.first_difference(w1, w1_f, lay) is None, TR.first_difference(w1, w1_f, lay)
        # ---- the single-GPU engine started from those same weights
        loss1, g1, w1_one = single_step(w0, mb)
        worst = _rel_l2_worst(blocks, g, g1)
        w_one, _, _ = TR.tf_adam(w0, g1, m, v, step + 1, k)       # Adam on the moments the group's own gradients left, on the single-GPU gradients
        _, m, v = TR.tf_adam(w0, g, m, v, step + 1, k)
        dw = np.abs(w1 - w_one)[tr]
        print(f"world 8 x 64 records, step {step}: losses off by {abs(loss[0] - loss1[0]):.1e} / {abs(loss[1] - loss1[1]):.1e}, worst per-tensor "
              f"relative L2 gradient difference {worst:.2e}, median |dw| {np.median(dw):.1e}, share of |dw| > 2e-5 {(dw > 2e-5).mean():.1e}, "
              f"{per_step} all-reduces per step")
        assert np.abs(np.array(loss) - np.array(loss1)).max() <= 2e-5, (step, loss, loss1)
        assert worst <= 3e-3, (step, worst)
        assert np.median(dw) <= 2e-7 and (dw > 2e-5).mean() <= 5e-3, (step, np.median(dw), (dw > 2e-5).mean())
        if fresh_state:
            # both sides on cleared optimiser state: the single-GPU engine's own Adam step, as this test has always compared it
            dw = np.abs(w1 - w1_one)
            moved = np.abs(w1_one - flat) > 0
            assert np.median(dw[moved]) <= 2e-7 and (dw[moved] > 2e-5).mean() <= 5e-3, (np.median(dw[moved]), (dw[moved] > 2e-5).mean())
        # ---- measured only: the single-GPU trajectory
        w_ref0 = ref.get_weights()
        loss_r = ref.train_batch(mb)
        g_r = ref.train_grads()
        if not fresh_state:
            apart = np.abs(w0 - w_ref0)[tr]
            _, g_from_ref, _ = single_step(w_ref0, mb)    # == g_r bit for bit: a step is a function of weights and minibatch
            assert TR.first_difference(g_from_ref, g_r, lay) is None
            print(f"  cause of the step-2 difference between the trajectories (measured): {int(((apart > 1e-3) & (apart < 3e-3)).sum())} of "
                  f"{int(tr.sum())} trained weights differ by about 2e-3 after step 1 (Adam's first step on a gradient whose sign the "
                  f"summation order decides), {int((apart > 2e-5).sum())} by more than 2e-5; step 2 gradients, trajectory against "
                  f"trajectory: {_rel_l2_worst(blocks, g, g_r):.2e} relative L2 (losses {abs(loss[0] - loss_r[0]):.1e} / {abs(loss[1] - loss_r[1]):.1e}); "
                  f"single-GPU step 2 from the group's weights against single-GPU step 2 from the trajectory's weights — the weight "
                  f"difference alone —: {_rel_l2_worst(blocks, g1, g_r):.2e}; group against single-GPU from the SAME weights: {worst:.2e}")
    worst_adam = TR.adam_trajectory(trace, k)
    print(f"  adam_trajectory over both steps: worst deviation {worst_adam:.2e} (bound {TR.ADAM_BOUND:.0e})")
    group.close()
    ref.close()


def test_bench_five_ranks_over_gloo():
    """`python bench.py --gpus 5` (its own spawner: a parent that never touches HIP starts the ranks) with the gloo rehearsal backend:
    5 disjoint seed streams, weak-scaling totals, the padded record gather of 5 ragged counts"""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "5", "--games", "16", "--sims", "8", "--blocks", "1", "--steps", "2",
           "--warmup", "1", "--full", "--no-extra", "--no-cpu-baseline", "--tail-seconds", "40"]
    r = subprocess.run(cmd, env=_env(AZR_BENCH_BACKEND="gloo", AZR_BENCH_DEADLINE_S="600"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:] + r.stdout[-1000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["n_gpus"] == 5 and out["scaling"] == "weak" and out["value"] > 0 and out["errors"] == 0 and out["records_dropped"] == 0
    ex = out["exchange"]
    assert "backend gloo" in ex["collective"] and ex["records_gathered"] > ex["records_this_rank"] > 0
    assert ex["bytes"] == 265 * ex["records_gathered"]
    # every rank ran its own games and contributed its records
    assert ex["records_gathered"] >= 3 * ex["records_this_rank"] and 0.9 <= out["decisions_per_game_and_step"] <= 2.0, out


@pytest.mark.parametrize("dp", ["1", "0"])
def test_learn_iteration_four_ranks_ragged_over_gloo(tmp_path, dp):
    """one learn.py iteration at world 4 over gloo (ranks share the card; with the runner and torchrun's agent that is the box's 6
    processes): 7 self-play games over 4 ranks (2, 2, 2, 1), record gather of 4 ragged counts, training — the data-parallel step with
    16-record shares of a 64-record minibatch (--dp 1) or rank 0 + weight broadcast (--dp 0, the default) —, 3 compare pairs over 4
    ranks (one rank plays nothing and contributes an EMPTY record shard), 5 + 50 benchmark pairs split, GameResults reduced, rank 0
    writes the reference's files"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
           "--master-port", str(_port()), os.path.join(ROOT, "alphazero-risk_amd", "learn.py"), "--ti", "1", "--tg", "7", "--mcts", "6",
           "--gpu-games", "8", "--blocks", "1", "-e", "2", "--bs", "64", "--cg", "6", "--ct", "0", "--dp", dp, "--phase-deadline", "600"]
    r = subprocess.run(cmd, cwd=tmp_path, env=_env(AZR_LEARN_BACKEND="gloo"), capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:] + r.stdout[-2000:]
    assert "world 4" in r.stdout and "Model improved" in r.stdout and "Loss Policy / Value" in r.stdout
    assert ("Data-parallel optimiser step" in r.stdout) == (dp == "1")
    assert ("Weight broadcast from rank 0" in r.stdout) == (dp == "0")
    assert "[7 games," in r.stdout
    imp = open(tmp_path / "log/azr-improvement-log.txt").read().strip().split(",")
    assert imp[0] == "0" and int(imp[1]) + int(imp[2].split("/")[0]) + int(imp[3].split("/")[0]) == 6
    bench = open(tmp_path / "log/azr-benchmark-log.txt").read().strip()
    nums = [int(x.split("/")[0]) for x in bench.replace(" ", "").split(",")[1:]]
    assert nums[0] + nums[1] + nums[2] == 10 and nums[3] + nums[4] + nums[5] == 100
    raw = open(tmp_path / "data/training_samples.bin", "rb").read()
    n = int(np.frombuffer(raw[:8], np.uint64)[0])
    assert len(raw) == 8 + n * 265 and n > 500


def _host_exe():
    subprocess.check_call(["make", "-s", "-C", HOST])
    return EXE


def test_host_cli_train_two_gpus_on_one_card(tmp_path):
    """`AlphaZero_Risk_hip -m train --gpus 2 --devices 0,0 --ti 1`: the C++ host's in-process multi-GPU path — one host thread per GPU
    for self-play (disjoint seed streams, storages concatenated in GPU order), GPU 0 trains and hands the weights to GPU 1 through
    checkpoints/temp.bin, the compare pairs and the benchmark pairs split over both GPUs, results merged"""
    exe = _host_exe()
    cmd = [exe, "-m", "train", "--gpus", "2", "--devices", "0,0", "--ti", "1", "--tg", "9", "--mcts", "6", "--gpu-games", "8", "--blocks", "1",
           "-e", "1", "--bs", "64", "--cg", "10", "--ct", "0", "-t", "2"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    out = r.stdout
    assert "GPUs: 2" in out and "Model improved" in out
    assert "[gpu 0] games 5/5" in out and "[gpu 1] games 4/4" in out          # 9 games: 5 + 4
    assert "Self-play: 9 games" in out
    assert os.path.exists(tmp_path / "checkpoints/temp.bin")                      # AlphaZeroNNGroup::train's hand-over file
    imp = open(tmp_path / "log/azr-improvement-log.txt").read().strip().split(",")
    assert imp[0] == "0" and int(imp[1]) + int(imp[2].split("/")[0]) + int(imp[3].split("/")[0]) == 10   # 5 pairs: 3 + 2
    bench = open(tmp_path / "log/azr-benchmark-log.txt").read().strip()
    nums = [int(x.split("/")[0]) for x in bench.replace(" ", "").split(",")[1:]]
    assert nums[0] + nums[1] + nums[2] == 10 and nums[3] + nums[4] + nums[5] == 100
    # GPU 0's trained weights = the hand-over file = the accepted checkpoint every GPU of the generate group then loaded
    assert open(tmp_path / "checkpoints/best-checkpoint.bin", "rb").read() == open(tmp_path / "checkpoints/temp.bin", "rb").read()


def test_host_cli_play_two_gpus_on_one_card(tmp_path):
    """`-m play --gpus 2 --devices 0,0`: the game quota split in whole pairs over two host threads, results merged; an engine that
    cannot be created ends the CLI with exit code 1 and the engine's message (failures INSIDE the per-GPU threads:
    tests/test_host_threads.py)"""
    exe = _host_exe()
    r = subprocess.run([exe, "-m", "play", "--gpus", "2", "--devices", "0,0", "--mcts=8", "--cg=12", "--blocks=1", "--gpu-games", "4"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    tail = r.stdout.strip().split("\n")[-4:]
    assert tail[0] == "Games: 12" and sum(int(t.split(":")[1]) for t in tail[1:]) == 12
    bad = subprocess.run([exe, "-m", "play", "--gpus", "2", "--devices", "0,99", "--mcts=8", "--cg=4", "--blocks=1"], cwd=tmp_path, capture_output=True,
                         text=True, timeout=600)
    assert bad.returncode == 1 and "fatal:" in bad.stderr and "terminate" not in bad.stderr, (bad.returncode, bad.stderr[-500:])
