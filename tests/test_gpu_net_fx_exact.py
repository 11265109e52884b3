"""NET_F32X (csrc/azr_tower_fx.hip, k_tower_fx<2>) against an exact model of the fp16 pair (tests/precision_ref.forward_fx), not
against the fp32 oracle.

On a lattice net of the pair (precision_ref.lattice_net_fx) every product ah wh, al wh, ah wl and every fp32 partial sum of the
tower is exact, so the tower's fp32 activations are one set of bits whatever the MFMA order; a fragment that is missing, lands in
another accumulator or is read one k-slice late meets a non-zero operand somewhere (tests/test_precision_ref.py shows both, and
that each such mistake in ONE fragment position moves pi or v by 4 x the tolerance or more).  What is left against the model's
float64 heads is the fp32 noise of fused_heads, the same heads as the 16-bit towers': tolerance precision_ref.GPU_TOL = 5e-6.
Measured on the MI355X: see MEASURED below."""
import numpy as np
import pytest

import precision_ref as M
from gpu_common import pkg

pytestmark = pytest.mark.gpu

MEASURED = "not yet recorded"
SIZES = [1, 2, 3, 17, 64, 257]   # one tile shape (2 boards per workgroup): the odd tail, first and last workgroups


def engine(P, blocks, flat, games):
    eng = P.Engine(games, blocks=blocks, sims=1, dtype=P.NET_F32X, node_capacity=64)
    eng.set_weights(flat)
    return eng


def compare(eng, x, rpi, rv, what):
    pi, v = eng.predict(x)
    dpi, dv = float(np.abs(pi - rpi).max()), float(np.abs(v - rv).max())
    print(f"f32x {what}: max |d pi| {dpi:.2e}, max |d v| {dv:.2e}")
    assert dpi <= M.GPU_TOL and dv <= M.GPU_TOL, (what, dpi, dv)
    return dpi, dv


@pytest.mark.parametrize("blocks", [1, 2, 20])
def test_f32x_lattice_net(blocks):
    """the lattice net on launches of 1 .. 257 boards, each filled from the pool of 256 boards in its own seeded permutation (every
    board meets both slots of a workgroup and other partners); every board of every launch against the model"""
    P = pkg()
    flat, x, rpi, rv, _ = M.fx_pool(blocks)
    eng = engine(P, blocks, flat, max(SIZES))
    rng = np.random.default_rng(blocks)
    worst = [0.0, 0.0]
    for n in SIZES:
        idx = np.concatenate([rng.permutation(len(x)) for _ in range(-(-n // len(x)))])[:n]
        d = compare(eng, x[idx], rpi[idx], rv[idx], f"B={blocks} n={n}")
        worst = [max(worst[0], d[0]), max(worst[1], d[1])]
    print(f"f32x B={blocks}: max |d pi| {worst[0]:.2e}, max |d v| {worst[1]:.2e} over {len(SIZES)} launches")
    eng.close()


def test_f32x_batch_invariance_bit_for_bit():
    """the same board alone, as board 0 and as board 1 of a workgroup, and in the last, half-empty workgroup of an odd launch:
    identical pi / v bits"""
    P = pkg()
    blocks = 2
    flat, x, _, _, _ = M.fx_pool(blocks)
    eng = engine(P, blocks, flat, 8)
    for i in (0, 1, 2):
        b, other = x[i:i + 1], x[10 + i:13 + i]
        alone = eng.predict(b)
        for what, batch, at in (("board 0", np.concatenate([b, other[:1]]), 0), ("board 1", np.concatenate([other[:1], b]), 1),
                                ("last workgroup of 3", np.concatenate([other[:2], b]), 2),
                                ("last workgroup of 5", np.concatenate([other, other[:1], b]), 4)):
            pi, v = eng.predict(batch)
            assert (pi[at].view(np.uint32) == alone[0][0].view(np.uint32)).all(), (i, what)
            assert v[at:at + 1].view(np.uint32) == alone[1][:1].view(np.uint32), (i, what)
    eng.close()


def test_f32x_stem_keeps_fp32_planes():
    """float planes that fp16 cannot represent (ties between fp16 neighbours among them): the stem runs on the fp32-input MFMA and
    the model keeps them in fp32 (rounding them first moves the outputs: test_fx_edge_and_stem_nets_pass_the_certificate)"""
    P = pkg()
    blocks = 2
    flat = M.lattice_net_fx(blocks, 6, stem_fine=0)
    x = M.fx_boards(96, 10, exact_planes=False)
    rpi, rv, _ = M.forward_fx(flat, blocks, x, certify=True)
    eng = engine(P, blocks, flat, 97)
    rng = np.random.default_rng(4)
    for n in (1, 2, 97):
        idx = rng.permutation(np.tile(np.arange(len(x)), 2))[:n]
        compare(eng, x[idx], rpi[idx], rv[idx], f"non-representable planes n={n}")
    eng.close()


@pytest.mark.parametrize("kind", ["scale_clamps", "subnormal_wl"])
def test_f32x_layer_scale_edges(kind):
    """net_fx_upload's layer scale at both clamps (e = 24, e = -2) and on an all-zero layer (e = 0); a layer whose smallest rich
    weights have subnormal low parts, which the matrix core takes at full value (precision_ref.fx_edge_net)"""
    P = pkg()
    flat = M.fx_edge_net(kind, 5)
    x = M.fx_boards(64, 11)
    rpi, rv, _ = M.forward_fx(flat, 2, x, certify=True)
    eng = engine(P, 2, flat, 65)
    rng = np.random.default_rng(3)
    for n in (3, 65):
        idx = rng.permutation(np.tile(np.arange(len(x)), 2))[:n]
        compare(eng, x[idx], rpi[idx], rv[idx], f"{kind} n={n}")
    eng.close()
