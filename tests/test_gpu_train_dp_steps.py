"""GPU: the data-parallel optimiser step (azr_nn_train_dp through a callback) in every kernel family and at every step of a group's
life, on groups of ranks in ONE process (tests/dp_group.py: one handle and one host thread per rank, sums in rank order, so a group's
step is deterministic to the bit; its own checks run on the CPU in tests/test_dp_group.py).
  1. the FIRST step of a group against the float64 graph on the whole minibatch (torch_train_ref.torch_step), under the bounds of
     test_gpu_train.py::test_step_matches_torch_graph, with shares in all three families of ctx_ensure's plan — the fp32-MFMA GEMMs
     (share % 16 != 0), t_conv_q with the weight gradient on the side stream (<= 128), t_conv_rs (> 128: t_sum_slices and
     t_bn_bwd_finalize on the reduced slab instead of t_sum_slices_fin) —, the smallest legal share, worlds that are no power of two,
     one rank with a callback; which records a rank took is pinned by its own contribution to the loss sum;
  2. every later step — behind other shares, validation passes, a plain single-GPU step on the same handles, a reset — replayed on a
     fresh group, bit for bit (train_replay.assert_pure), Adam's state restated on the host (adam_trajectory);
  3. azr_nn_train_dp's queue of steps against single steps driven by libstdc++'s own shuffle.
The product library (no test hooks), NET_F32, weights make_net_flat(blocks, seed=11, perturb_bn=True) unless stated.
Measured figures: profiles/train_dp_measured.txt."""
import functools

import numpy as np
import pytest

import azr_testlib as T
import dp_group as DG
import torch_train_ref as train
import train_replay as TR
from gpu_common import pkg, records
from torch_train_ref import torch_step

pytestmark = pytest.mark.gpu


def _engine(blocks):
    P = pkg()
    return lambda: P.Engine(8, blocks=blocks, sims=1, dtype=P.NET_F32, node_capacity=64)


def _group(world, blocks):
    return lambda: DG.DpGroup(world, _engine(blocks))


def _per_step(blocks):
    """2 all-reduces per batch-norm layer (L conv layers + the heads: statistics forward, their two sums backward), the loss pair, the gradient"""
    return 2 * (2 * blocks + 1 + 1) + 2


@functools.lru_cache(maxsize=None)
def _filtered_reference(blocks, bs):
    """(record seed, smallest |ReLU input|, records, float64 step, per-record terms) for the first record seed of blocks + 1 ..
    blocks + 32 whose float64 forward keeps every ReLU input at least 1e-6 from zero (as test_step_matches_torch_graph searches);
    computed once per process, callers must not write into it"""
    flat = T.make_net_flat(blocks, seed=11, perturb_bn=True)
    for seed in range(blocks + 1, blocks + 33):
        rec = records(bs, seed=seed)
        margin = []
        torch_step(blocks, flat, rec, margin, backward=False)
        if min(margin) >= 1e-6:
            terms = []
            return seed, min(margin), rec, torch_step(blocks, flat, rec, per_record=terms), terms
    pytest.fail("no record seed with a ReLU margin of 1e-6")


def _group_step(world, blocks, flat, rec, terms):
    """one step of a fresh group; returns (losses, gradients, weights behind it, the rows of DG.membership); the checks every case
    shares are made here: ranks bit-equal (get_weights / train_grads assert that), the all-reduce count, which records a rank took"""
    group = _group(world, blocks)()
    try:
        group.set_weights(flat)
        loss = group.train_batch(rec)
        g, w1 = group.train_grads(), group.get_weights()
        DG.assert_calls(group, 1, _per_step(blocks), len(flat))
        rows = DG.membership(group.loss_parts(), terms[0], terms[1])
        print("  membership (rank, term, rank's contribution x batch, float64 sum of its slice): " +
              ", ".join("(%d, %s, %.7g, %.7g)" % (r, "pv"[k], got, want) for r, k, got, want in rows))
        member = DG.assert_membership(group.loss_parts(), terms[0], terms[1])
    finally:
        group.close()
    return loss, g, w1, member


# (world, blocks, batch, record seed the search must arrive at)
ROWS = [(5, 1, 10, 3),      # share 2: fp32-MFMA GEMMs, the smallest legal share
        (3, 1, 30, 3),      # share 10: fp32, a world that is no power of two
        (2, 2, 20, 6),      # share 10: fp32, two blocks
        (4, 2, 32, 4),      # share 8: fp32 share of a batch that is t_conv_q on one GPU
        (4, 1, 64, 7),      # share 16: t_conv_q, the smallest
        (2, 1, 96, 18),     # share 48: t_conv_q, partial last board group
        (2, 2, 64, 7),      # share 32: t_conv_q, two dY sets
        (2, 1, 160, 2),     # share 80: t_conv_q share of a batch that is t_conv_rs on one GPU
        (1, 1, 160, 2),     # t_conv_rs, one rank with a callback
        (1, 1, 10, 3)]      # fp32, one rank with a callback


@pytest.mark.parametrize("world,blocks,bs,want_seed", ROWS)
def test_first_dp_step_matches_torch_graph(world, blocks, bs, want_seed):
    """bounds of test_step_matches_torch_graph, unchanged: losses 2e-5, every gradient tensor within 2e-3 of its largest entry, moving
    statistics rtol 2e-5 / atol 1e-6, tf_adam on the group's own gradients within 2e-7; membership 2e-5 times the share"""
    flat = T.make_net_flat(blocks, seed=11, perturb_bn=True)
    seed, margin, rec, (rlp, rlv, rg, rflat), terms = _filtered_reference(blocks, bs)
    (lp, lv), g, w1, member = _group_step(world, blocks, flat, rec, terms)
    k = TR.kinds(blocks)
    errs = {}
    for name, off, shape in train.layout(blocks)[0]:
        n = int(np.prod(shape)) if not name.endswith("_bn") else 2 * shape[1]
        a, b = g[off:off + n].astype(np.float64), rg[off:off + n]
        scale = max(np.abs(b).max(), 1e-6)
        errs[name] = (np.abs(a - b).max() / scale, int((np.abs(a - b) > 2e-3 * scale).sum()), scale)
    worst = max(errs, key=lambda name: errs[name][0])
    w_ref, _, _ = TR.tf_adam(flat, g, np.zeros_like(flat), np.zeros_like(flat), 1, k)
    adam = np.abs(w1[k > 0] - w_ref[k > 0]).max()
    print(f"(world {world}, {blocks} blocks, {bs} -> {bs // world}): record seed {seed}, smallest |ReLU input| {margin:.2e}, losses off by "
          f"{abs(lp - rlp):.1e} / {abs(lv - rlv):.1e}, worst gradient error {errs[worst][0]:.2e} of the largest entry in {worst}, "
          f"membership {member:.1e} (bound {2e-5 * (bs // world):.1e}), Adam {adam:.1e}")
    for name, (err, beyond, scale) in errs.items():
        print(f"    {name}: {err:.2e} ({beyond} entries beyond 2e-3 of {scale:.2e})")
    assert seed == want_seed, (seed, want_seed)
    assert abs(lp - rlp) <= 2e-5 * max(1, abs(rlp)) and abs(lv - rlv) <= 2e-5, (lp, rlp, lv, rlv)
    for name, (err, beyond, scale) in errs.items():
        assert err <= 2e-3, (name, err, beyond, scale)
    assert np.allclose(w1[k == 0], rflat[k == 0], rtol=2e-5, atol=1e-6)
    assert adam <= 2e-7, adam


@functools.lru_cache(maxsize=None)
def _unfiltered_reference(blocks, bs):
    flat = T.make_net_flat(blocks, seed=21, perturb_bn=True)
    rec = records(bs, seed=77)
    terms = []
    return flat, rec, torch_step(blocks, flat, rec, per_record=terms), terms


def _l2_per_kernel(blocks, g, rg):
    out = {}
    for name, off, shape in train.layout(blocks)[0]:
        if name.endswith("_w"):
            n = int(np.prod(shape))
            out[name] = np.linalg.norm(g[off:off + n].astype(np.float64) - rg[off:off + n]) / np.linalg.norm(rg[off:off + n])
    return out


@pytest.mark.parametrize("world,blocks,bs", [(2, 2, 512), (2, 1, 320)])
def test_t_conv_rs_shares_at_the_reference_measure(world, blocks, bs):
    """shares of 256 and 160 records: t_conv_rs under DP.  At these sizes no record seed keeps every ReLU input 1e-6 from zero, so the
    measure is the one of test_conv_kernel_families_at_the_reference_batch (weights seed 21, records(bs, seed=77)): the relative L2
    error per kernel tensor against float64, 3e-3 for stem and block kernels, 1e-5 for head tensors, losses 2e-5.  That measure was
    taken on one GPU at 512 records, so the single-GPU engine runs the same inputs as a control, and both have to meet it."""
    flat, rec, (rlp, rlv, rg, _), terms = _unfiltered_reference(blocks, bs)
    (lp, lv), g, w1, member = _group_step(world, blocks, flat, rec, terms)
    one = _engine(blocks)()
    one.set_weights(flat)
    lp1, lv1 = one.train_batch(rec)
    g1 = one.train_grads()
    one.close()
    e_dp, e_one = _l2_per_kernel(blocks, g, rg), _l2_per_kernel(blocks, g1, rg)
    print(f"(world {world}, {blocks} blocks, {bs} -> {bs // world}): losses off by {abs(lp - rlp):.1e} / {abs(lv - rlv):.1e} "
          f"(one GPU: {abs(lp1 - rlp):.1e} / {abs(lv1 - rlv):.1e}), membership {member:.1e} (bound {2e-5 * (bs // world):.1e})")
    for name in e_dp:
        print(f"    {name}: relative L2 {e_dp[name]:.2e} (one GPU: {e_one[name]:.2e})")
    for tag, e, l in (("one GPU", e_one, (lp1, lv1)), ("data-parallel", e_dp, (lp, lv))):
        assert abs(l[0] - rlp) <= 2e-5 * max(1, abs(rlp)) and abs(l[1] - rlv) <= 2e-5, (tag, l, rlp, rlv)
        for name, err in e.items():
            assert err <= (3e-3 if name[0] in "sb" else 1e-5), (tag, name, err)   # stem / block kernels | head tensors


SCHEDULES = {
    # shares of 32 (t_conv_q, side stream), 160 (t_conv_rs), 10 (fp32), 48 (t_conv_q, partial last group); a validation pass between
    # steps of one share, the plain single-GPU step on handles that have run DP steps (and DP steps behind it), a prediction, a reset
    2: [("train", 64), ("train", 64), ("validate", 48, 2), ("train", 64), ("train", 320), ("train", 320), ("solo", 64), ("train", 320),
        ("train", 20), ("train", 20), ("predict", 8), ("train", 96), ("reset",), ("train", 96), ("train", 64)],
    # shares of 16, 10 and 32 in a world that is no power of two
    3: [("train", 48), ("train", 48), ("train", 30), ("validate", 30, 1), ("train", 30), ("train", 96), ("reset",), ("train", 48)],
}


@pytest.mark.parametrize("world", [2, 3])
def test_every_dp_step_is_a_pure_function_of_weights_and_batch(world):
    """what the single-GPU step's replay proves, for a group: whatever the step, the share, the call before left in the ranks' training
    contexts — cur[0] and the rank offset cur[2], the step count, m / v handed over when the context is rebuilt for another share, the
    two dY sets and their events, world / rank / callback of an earlier call — every step is the function of weights and minibatch
    that the first step of a fresh group is, bit for bit; Adam's moments and step count survive everything but the reset."""
    blocks = 2
    schedule = SCHEDULES[world]
    need = sum((s[1] * s[2] if s[0] == "validate" else s[1]) for s in schedule if len(s) > 1)
    make = _group(world, blocks)
    trace = TR.run_schedule(make, T.make_net_flat(blocks, seed=11, perturb_bn=True), schedule, records(need, seed=31))
    TR.assert_pure(trace, TR.replay(make, trace))
    worst = TR.adam_trajectory(trace, TR.kinds(blocks))
    steps = [s for s in trace if s.kind in TR.TRAIN_KINDS]
    print("world %d: adam_trajectory over %d steps: worst deviation %.2e (bound %.0e)" % (world, len(steps), worst, TR.ADAM_BOUND))
    assert all(np.abs(s.w1 - s.w0).max() > 1e-4 for s in steps)


@pytest.mark.parametrize("world,bs", [(2, 64), (3, 30), (2, 320)])
def test_dp_epoch_loop_equals_dp_single_steps(world, bs):
    """azr_nn_train_dp queues floor(n / bs) steps per epoch back to back — t_tick_batch moves cur[0] by the WHOLE batch, cur[2] stays the
    rank's offset —: 2 epochs over 3 * bs + 8 records against DpGroup.train_batch driven by the probe's permutations; epoch losses ==,
    weights equal as uint32 on every rank"""
    blocks, n = 1, 3 * bs + 8
    DG.epoch_loop_against_single_steps(_group(world, blocks), T.make_net_flat(blocks, seed=4), records(n, seed=6), bs, 2, 20260003)
