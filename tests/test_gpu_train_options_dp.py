"""GPU: the optimiser step's options under azr_nn_train_dp, on a group of two ranks in one process (tests/dp_group.py: sums in rank
order, so the group's step is deterministic to the bit).  The norm is taken behind the gradient all-reduce: every rank computes the
same norm, clip scale, rate and EMA, so their weights, EMA vectors and stats stay equal without a broadcast."""
import numpy as np

import pytest

import azr_testlib as T
import dp_group as DG
import train_options_ref as R
import train_replay as TR
from gpu_common import pkg, records

pytestmark = pytest.mark.gpu

f32 = np.float32
BLOCKS, BS = 1, 32        # 16 records per rank: t_conv_q


def test_two_ranks_clip_schedule_and_ema_alike():
    """clipping (to half the first step's norm, taken in advance from a single engine on default options: the same gradient up to the
    order of the sums), the cosine schedule and the EMA, two steps of 32 records: the group's own rank-equality check passes for the
    weights, the gradients and the EMA vectors, the ranks' stats are equal as bytes, and the weights are within ADAM_BOUND of the
    restated Adam on the reduced gradients"""
    P = pkg()
    flat, rec, k = T.make_net_flat(BLOCKS, seed=11, perturb_bn=True), records(2 * BS, seed=43), TR.kinds(BLOCKS)
    tr = k > 0
    solo = P.Engine(8, blocks=BLOCKS, sims=1, dtype=P.NET_F32, node_capacity=64)
    solo.set_weights(flat)
    solo.train_batch(rec[:BS])
    clip = float(f32(0.5 * R.grad_norm(flat, solo.train_grads(), k, 1e-3)))
    solo.close()
    opts = dict(lr_schedule=R.LR_COSINE, warmup_steps=1, total_steps=3, lr_min=1e-4, clip_norm=clip, ema_decay=0.75)
    o = R.options(**opts)

    def make_engine():
        e = P.Engine(8, blocks=BLOCKS, sims=1, dtype=P.NET_F32, node_capacity=64)
        e.train_set_options(**opts)
        return e

    group = DG.DpGroup(2, make_engine)
    try:
        group.set_weights(flat)
        m, v, e_prev, clipped = np.zeros(len(k), f32), np.zeros(len(k), f32), flat, 0
        for t in (1, 2):
            w0 = group.get_weights()
            group.train_batch(rec[(t - 1) * BS:t * BS])
            g, w1 = group.train_grads(), group.get_weights()               # (each asserts that the ranks hold the same bits)
            ema = group._agree("get_ema_weights", group._each("get_ema_weights", lambda r, e: e.get_ema_weights()))
            stats = group._each("train_stats", lambda r, e: e.train_stats())
            group._agree("train_stats", [np.array([s[f] for f in sorted(s)], np.float64) for s in stats])
            st = stats[0]
            norm = R.grad_norm(w0, g, k, o["l2"])
            s = R.clip_scale(norm, clip)
            clipped += int(s < 1)
            assert st["step"] == t and st["ema_steps"] == t and st["clipped_steps"] == clipped and (t > 1 or 0.4 < st["clip_scale"] < 0.6)
            assert abs(st["grad_norm"] - norm) <= 5e-7 * norm and abs(st["clip_scale"] - float(s)) <= 2 * float(np.spacing(s))
            assert abs(st["lr"] - R.lr_eff(t, o)) <= float(np.spacing(f32(st["lr"])))
            w, m, v = R.adam(w0, g, m, v, k, R.lr_t(t, o), o["l2"], s)
            dev = float(np.abs(w1[tr] - w[tr]).max())
            print("step %d: clip_scale %.6f, lr %.6g, weights %.2e from the restated Adam (bound %.0e)" % (t, st["clip_scale"], st["lr"], dev, TR.ADAM_BOUND))
            assert dev <= TR.ADAM_BOUND
            want = R.ema(e_prev, w1, k, 0.75)
            assert (np.abs(ema - want) <= 2.0 ** -22 * np.maximum(np.abs(e_prev), np.abs(w1))).all()
            e_prev = ema
    finally:
        group.close()
