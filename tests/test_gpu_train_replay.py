"""GPU: every optimiser step, validation pass and prediction of a long-lived engine replayed on a fresh engine, bit for bit
(tests/train_replay.py; its own checks run on the CPU in tests/test_train_replay.py).  test_gpu_train.py compares the FIRST step of an
engine with the float64 graph; here every later step — behind other batch sizes, kernel families, validation passes, a reset — must be
the same function of weights and minibatch that the first step is, and Adam's state must survive everything but the reset.
The product library (no test hooks) throughout; weights make_net_flat(2, seed=11, perturb_bn=True) unless stated."""
import functools

import numpy as np
import pytest

import azr_testlib as T
import train_replay as TR
from gpu_common import pkg, records

pytestmark = pytest.mark.gpu

BLOCKS = 2   # two blocks: the side-stream weight-gradient branch alternates its two dY sets and the chain waits on ev_wg for layer l + 2


def _maker(dtype_name, blocks=BLOCKS):
    P = pkg()
    return lambda: P.Engine(8, blocks=blocks, sims=1, dtype=getattr(P, dtype_name), node_capacity=64)


def _flat():
    return T.make_net_flat(BLOCKS, seed=11, perturb_bn=True)


def test_every_step_is_a_pure_function_of_weights_and_batch():
    """NET_F32, one engine through four batch sizes, one per path of ctx_ensure's plan:
      64 records:  t_conv_q, the weight gradient on the side stream: 13 five-board slices, the last of 4 boards; 4 partials of 4, 4, 4, 1 slices
      160 records: t_conv_rs on one stream with t_sum_slices_fin: 16 ten-board slices
      50 records:  2100 rows, no multiple of the 32-deep k-tile: the fp32-MFMA GEMMs for every layer, split-K of 3 slices of 704 rows
      48 records:  t_conv_q, 10 slices, the last of 3 boards, partials of 4, 4, 2; the stem's split-K 2 x 1024 over 2016 rows
    A validation pass at the training batch size (it overwrites mean / istd / hstat with the moving statistics and repacks wpf) and one at
    another (two context rebuilds that must carry m, v and the step count) sit between steps of one size; a prediction reads the
    refreshed inference image; a reset clears the optimiser state, so the step behind it equals a fresh engine's in every weight."""
    schedule = [("train", 64), ("train", 64), ("validate", 64, 2), ("train", 64),
                ("train", 160), ("train", 160), ("validate", 48, 2), ("train", 160),
                ("train", 50), ("train", 50), ("predict", 8),
                ("train", 48), ("reset",), ("train", 48), ("train", 64)]
    make = _maker("NET_F32")
    trace = TR.run_schedule(make, _flat(), schedule, records(1164, seed=31))
    TR.assert_pure(trace, TR.replay(make, trace))
    worst = TR.adam_trajectory(trace, TR.kinds(BLOCKS))
    print("adam_trajectory over %d steps: worst deviation %.2e (bound %.0e)" % (sum(s.kind == "train" for s in trace), worst, TR.ADAM_BOUND))
    # the schedule did train: every step moved the weights by about the learning rate
    assert all(np.abs(s.w1 - s.w0).max() > 1e-4 for s in trace if s.kind == "train")


INFER_SCHEDULE = [("train", 64), ("predict", 8), ("train", 160), ("predict", 8), ("train", 50), ("predict", 8)]


@functools.lru_cache(maxsize=None)
def _infer_run(dtype_name):
    """the trace of INFER_SCHEDULE on an engine of this inference dtype (computed once per process; callers must not write into it)"""
    return tuple(TR.run_schedule(_maker(dtype_name), _flat(), INFER_SCHEDULE, records(64 + 160 + 50 + 24, seed=32)))


@pytest.mark.parametrize("dtype_name", ["NET_BF16", "NET_F16", "NET_F32X"])
def test_inference_images_follow_every_step(dtype_name):
    """finish -> net_upload after every step, in each family: NET_F16 derives its per-layer power-of-two scales from the new weights,
    NET_BF16 and NET_F32X repack; each prediction equals a fresh engine's that was given the weights of that moment.
    The step itself runs on the fp32 master copy (h->net.d_flat) whatever the inference dtype — azr_train.hip never reads
    cfg.net_dtype, and net_upload copies the same h->flat into d_flat for all four — so the three gradient vectors are those of a
    NET_F32 engine on the same schedule, bit for bit."""
    trace = _infer_run(dtype_name)
    TR.assert_pure(list(trace), TR.replay(_maker(dtype_name), trace))
    lay = TR.train.layout(BLOCKS)[0]
    for i, (a, b) in enumerate(zip(trace, _infer_run("NET_F32"))):
        if a.kind == "train":
            assert a.out == b.out, (i, a.out, b.out)
            assert TR.first_difference(a.grads, b.grads, lay) is None, (i, a.bs, TR.first_difference(a.grads, b.grads, lay))


@pytest.mark.parametrize("blocks,bs", [(1, 160), (1, 50)])
def test_epoch_loop_equals_single_steps_in_every_family(tmp_path, blocks, bs):
    """azr_nn_train queues its steps back to back with no host synchronisation between them; test_gpu_train.py runs that in the
    t_conv_q family (16 records).  Here t_conv_rs with t_sum_slices_fin (160) and the fp32-MFMA GEMMs (50): 2 epochs of 3 batches and a
    dropped remainder of 6 records, against train_batch driven by the same permutations."""
    n, state = 3 * bs + 6, 20260003
    a, st, end_state = TR.epoch_loop_against_single_steps(pkg(), tmp_path, blocks, bs, n, 2, state, T.make_net_flat(blocks, seed=4),
                                                          records(n, seed=6))
    a.close()
    assert st == end_state
