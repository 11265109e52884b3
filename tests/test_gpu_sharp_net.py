"""GPU: the heads (k_heads, fused_heads) on a net with the outputs of a trained one (azr_testlib.make_sharp_net_flat: policy logits
scaled by 2^8, value pre-activation centred and scaled by 2^10).  The other net tests run random-init heads, whose softmax stays
near 1/43 and whose tanh never saturates; here lv - mx runs below -87 (denormal quotients) and -104 (expf gives 0), one prior is
exactly 1 and tanhf returns +-1.  B = 1 and 2; 1, 2, 5, 13 boards (k_tower_sc), 129 (one board per workgroup), 300 (k_tower_sb).
Entry 43 of the device's 44-float policy row is not checked: no C-ABI call returns it."""
import functools
import os

import numpy as np
import pytest
import torch

import azr_testlib as T
import torch_train_ref as train
from gpu_common import pkg

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 5, 13, 129, 300)
N_MAX = SIZES[-1]
DTYPES = ("NET_F32", "NET_F32X", "NET_F16", "NET_BF16")
SEED = 11


def boards():
    return T.distinct_boards(N_MAX)


def forward(dtype_name, blocks, mode=None, single=0):
    """{n: (pi, v)} for every launch size; mode: AZR_TOWER_SB of the test-hook library (read once, at engine creation);
    single: also the first `single` boards one by one, under the key 0"""
    P = pkg()
    old = os.environ.get("AZR_TOWER_SB")
    if mode is not None:
        os.environ["AZR_TOWER_SB"] = mode
    try:
        eng = P.Engine(N_MAX, blocks=blocks, sims=1, dtype=getattr(P, dtype_name), node_capacity=64, test_hooks=mode is not None)
    finally:
        if mode is not None:
            if old is None:
                del os.environ["AZR_TOWER_SB"]
            else:
                os.environ["AZR_TOWER_SB"] = old
    eng.set_weights(T.make_sharp_net_flat(blocks, SEED))
    out = {n: eng.predict(boards()[:n].copy()) for n in SIZES}
    if single:
        one = [eng.predict(boards()[i:i + 1].copy()) for i in range(single)]
        out[0] = (np.concatenate([p for p, _ in one]), np.concatenate([v for _, v in one]))
    eng.close()
    for pi, v in out.values():
        pi.setflags(write=False)
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def plan_outputs(dtype_name, blocks):
    """the product library's outputs: computed once per net and type, shared, never modified"""
    return forward(dtype_name, blocks, single=13)


@functools.lru_cache(maxsize=None)
def float64_outputs(blocks):
    net = train.AzrNet(blocks, T.make_sharp_net_flat(blocks, SEED)).double()
    net.eval()
    with torch.no_grad():
        logits, v = net(torch.from_numpy(train.planes_from_in88(boards())).double())
    return torch.softmax(logits, 1).numpy(), v.numpy()


def same_bits(a, b):
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_sharp_outputs_are_a_policy_and_a_value(dtype_name, blocks):
    """finite, pi >= 0 with |sum pi - 1| <= 1e-5 (43 quotients of one fp32 sum: 43 half-ulps of at most 1 are 2.6e-6), |v| <= 1; and
    the regime: an exact zero in pi on at least half the boards"""
    out = plan_outputs(dtype_name, blocks)
    for n in SIZES:
        pi, v = out[n]
        assert pi.shape == (n, 43) and v.shape == (n,)
        assert np.isfinite(pi).all() and np.isfinite(v).all()
        assert (pi >= 0).all() and (np.abs(pi.astype(np.float64).sum(1) - 1) <= 1e-5).all()
        assert (np.abs(v) <= 1).all()
    pi, v = out[N_MAX]
    assert 2 * int((pi == 0).any(1).sum()) >= N_MAX
    print("%s B=%d, %d boards: an exact zero on %d, a denormal on %d, max pi == 1 on %d, v == 1 on %d, v == -1 on %d" % (
        dtype_name, blocks, N_MAX, (pi == 0).any(1).sum(), ((pi > 0) & (pi < T.FLT_MIN)).any(1).sum(), (pi.max(1) == 1).sum(),
        (v == 1).sum(), (v == -1).sum()))


@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_sharp_outputs_do_not_depend_on_the_batch(dtype_name, blocks):
    """a board's pi and v are the same bits at every launch size — across the three towers of the plan — and one by one: the oracle
    calls the device net back one board at a time (hip_eval) and must get what the batched search got"""
    out = plan_outputs(dtype_name, blocks)
    rpi, rv = out[N_MAX]
    for n in SIZES[:-1]:
        pi, v = out[n]
        assert same_bits(pi, rpi[:n]) and same_bits(v, rv[:n]), (dtype_name, blocks, n)
    pi, v = out[0]
    assert same_bits(pi, rpi[:len(pi)]) and same_bits(v, rv[:len(v)]), (dtype_name, blocks, "one by one")
    assert len(np.unique(rpi, axis=0)) > 3 and len(np.unique(rv)) > 3   # (not one answer for every board)


@pytest.mark.parametrize("mode", ["0", "2", "3", "4"], ids=["one-board", "4-board", "2-board", "3-board"])
@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("dtype_name", ["NET_BF16", "NET_F16"])
def test_sharp_tile_shapes_bit_identical(dtype_name, blocks, mode):
    """every forced tile shape gives the plan's bits: fused_heads against itself across the boards per workgroup and against the
    one-board kernel's epilogue, where expf underflows and tanhf saturates"""
    ref = plan_outputs(dtype_name, blocks)
    out = forward(dtype_name, blocks, mode)
    for n in SIZES:
        assert same_bits(out[n][0], ref[n][0]) and same_bits(out[n][1], ref[n][1]), (dtype_name, blocks, mode, n)


@pytest.mark.parametrize("blocks", [1, 2])
def test_sharp_fp32_accuracy_against_float64(blocks):
    """NET_F32 and NET_F32X against the float64 graph.  The bound is 8 x the error of the oracle's own fp32 CPU net against the same
    float64 evaluation on the same boards: what an independent fp32 evaluation in another summation order may differ by (the base
    net's gate of 2e-5 stands in that ratio to its measured 2.6e-6 / 4.5e-6).  A logit scale of 2^8 multiplies the tower's error
    into the softmax, so the figures are far from the base net's; they are printed, and kept in profiles/sharp_outputs_measured.txt."""
    rpi, rv = float64_outputs(blocks)
    opi, ov = T.orc_forward(blocks, T.make_sharp_net_flat(blocks, SEED), boards())
    e_pi, e_v = float(np.abs(opi - rpi).max()), float(np.abs(ov - rv).max())
    lines = ["B=%d %d boards: the oracle's fp32 net against float64: max |d pi| %.3e, max |d v| %.3e" % (blocks, N_MAX, e_pi, e_v)]
    got = {}
    for dtype_name in ("NET_F32", "NET_F32X"):
        pi, v = plan_outputs(dtype_name, blocks)[N_MAX]
        got[dtype_name] = (float(np.abs(pi - rpi).max()), float(np.abs(v - rv).max()))
        lines.append("B=%d %d boards: %s against float64: max |d pi| %.3e, max |d v| %.3e (bound 8 x the oracle's)" % (
            (blocks, N_MAX, dtype_name) + got[dtype_name]))
    print("\n".join(lines))
    assert e_pi > 0 and e_v > 0
    for dtype_name, (d_pi, d_v) in got.items():
        assert d_pi <= 8 * e_pi and d_v <= 8 * e_v, (dtype_name, d_pi, d_v, e_pi, e_v)
