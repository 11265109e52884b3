"""NET_BF16 / NET_F16 against an exact model (tests/precision_ref.py), not against the fp32 oracle.

On a lattice net (precision_ref.lattice_net) every product and every fp32 partial sum of the towers is exact, so summation order
does not matter: the tower's 16-bit output is one well-defined set of bits, which the CPU model computes with the kernels' rounding
points (stem features, weight packing and f16_scale, folded BN fma, shortcut add, ReLU, round to nearest even, fp16 saturation).
Every tile the planner can pick, every forced tile of the test hooks and both element types must reproduce it: what is left is the
fp32 noise of the heads against the model's float64 heads, tolerance precision_ref.GPU_TOL on pi and v.
Measured on the MI355X, every launch of test_lattice_net_on_every_tile (B = 20): max |d pi| 2.3e-6, max |d v| 2.9e-7 (bf16),
2.1e-6 / 2.4e-7 (f16) — the same in every mode; the other tests here stay below 1.5e-6 / 3.4e-7.  GPU_TOL = 5e-6."""
import numpy as np
import pytest

import precision_ref as M
from gpu_common import pkg

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 17, 113, 128, 129, 200, 256, 257, 400, 700, 1024, 2048]
# the product's plan for these sizes: (boards per workgroup, workgroups)
PLAN = {n: (2, (n + 1) // 2 * 4) for n in (1, 2, 17, 113, 128)}          # split-channel tower (k_tower_sc)
PLAN.update({n: (1, n) for n in (129, 200, 256)})                          # one board per workgroup (k_tower_bf16<1>)
PLAN.update({257: (2, 129), 400: (2, 200), 700: (3, 234), 1024: (4, 256), 2048: (4, 512)})   # k_tower_sb<2, 3, 4>
MODES = {"plan": {}, "SB=0": {"AZR_TOWER_SB": "0"}, "SB=2": {"AZR_TOWER_SB": "2"}, "SB=3": {"AZR_TOWER_SB": "3"},
         "SB=4": {"AZR_TOWER_SB": "4"}, "SC=0": {"AZR_TOWER_SC": "0"}}


def expected_plan(mode, n):
    """tower_plan(n) under the test hooks (csrc/azr_net_bf16.hip plan_sb and net_bf16_forward)"""
    if mode == "plan":
        return PLAN[n]
    if mode == "SB=0":
        return (1, n)
    if mode == "SC=0":
        return PLAN[n] if n > 256 else (1, n)
    snb = {"SB=2": 4, "SB=3": 2, "SB=4": 3}[mode]
    if n >= snb:
        return (snb, -(-n // snb))
    return PLAN[n]


_pools = {}


def pool(el):
    """512 distinct lattice boards and the model's pi, v for them on the B = 20 lattice net (certified), once per element type"""
    if el.name not in _pools:
        flat = M.lattice_net(20, 5, el)
        x = M.lattice_boards(512, 9, el)
        pi, v, _ = M.forward(flat, 20, x, el, certify=True)
        _pools[el.name] = (flat, x, pi, v)
    return _pools[el.name]


def engine(P, el, blocks, flat, games, env, monkeypatch):
    for k, val in env.items():
        monkeypatch.setenv(k, val)   # test hooks: read once, at creation, by libazr_hip_test.so only
    eng = P.Engine(games, blocks=blocks, sims=1, dtype=P.NET_BF16 if el is M.BF16 else P.NET_F16, node_capacity=64,
                   test_hooks=bool(env))
    for k in env:
        monkeypatch.delenv(k)
    eng.set_weights(flat)
    return eng


def compare(eng, x, rpi, rv, what):
    pi, v = eng.predict(x)
    dpi, dv = float(np.abs(pi - rpi).max()), float(np.abs(v - rv).max())
    assert dpi <= M.GPU_TOL and dv <= M.GPU_TOL, (what, dpi, dv)
    return dpi, dv


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("el", [M.BF16, M.F16], ids=lambda e: e.name)
def test_lattice_net_on_every_tile(monkeypatch, el, mode):
    """the B = 20 lattice net on launches of 1 .. 2048 boards, each filled from the pool of 512 boards in its own seeded permutation
    (every board meets other workgroup partners and slots in every launch); every board of every launch against the model"""
    P = pkg()
    flat, x, rpi, rv = pool(el)
    eng = engine(P, el, 20, flat, max(SIZES), MODES[mode], monkeypatch)
    rng = np.random.default_rng(len(mode))
    worst = [0.0, 0.0]
    for n in SIZES:
        assert eng.tower_plan(n) == expected_plan(mode, n), (mode, n, eng.tower_plan(n))
        idx = np.concatenate([rng.permutation(len(x)) for _ in range(-(-n // len(x)))])[:n]
        d = compare(eng, x[idx], rpi[idx], rv[idx], (el.name, mode, n))
        worst = [max(worst[0], d[0]), max(worst[1], d[1])]
    print(f"{el.name} {mode}: max |d pi| {worst[0]:.2e}, max |d v| {worst[1]:.2e} over {len(SIZES)} launches")
    eng.close()


@pytest.mark.parametrize("blocks", [1, 2, 20])
@pytest.mark.parametrize("el", [M.BF16, M.F16], ids=lambda e: e.name)
def test_stem_rounding(monkeypatch, el, blocks):
    """float planes the element type cannot represent (a third of them exact ties) behind a lattice stem: the stem features' round
    to nearest even (fp16: after the clamp at 65504), on the split-channel tower, one board per workgroup and the 2-board tile"""
    P = pkg()
    flat = M.lattice_net(blocks, 6, el)
    x = M.lattice_boards(96, 10, el, exact_planes=False)
    rpi, rv, _ = M.forward(flat, blocks, x, el, certify=True)
    eng = engine(P, el, blocks, flat, 300, {}, monkeypatch)
    rng = np.random.default_rng(blocks)
    for n in (1, 2, 96, 200, 300):
        idx = rng.permutation(np.tile(np.arange(len(x)), 4))[:n]
        dpi, dv = compare(eng, x[idx], rpi[idx], rv[idx], (el.name, blocks, n))
    print(f"{el.name} B={blocks} non-representable planes: max |d pi| {dpi:.2e}, max |d v| {dv:.2e} (last launch)")
    eng.close()


@pytest.mark.parametrize("kind", ["scale_clamps", "saturation", "subnormal"])
def test_f16_range_edges(monkeypatch, kind):
    """NET_F16 at the edges of its range (precision_ref.f16_edge_net): f16_scale at both clamps and on an all-zero layer,
    activations driven past 65504 (saturation at 0x7bff, bit for bit), and a tower that runs on fp16 subnormals"""
    P = pkg()
    flat = M.f16_edge_net(kind, 5)
    x = M.lattice_boards(256, 11, M.F16)
    rpi, rv, _ = M.forward(flat, 2, x, M.F16, certify=True)
    eng = engine(P, M.F16, 2, flat, 1024, {}, monkeypatch)
    rng = np.random.default_rng(3)
    for n in (2, 113, 200, 700, 1024):
        idx = rng.permutation(np.tile(np.arange(len(x)), 4))[:n]
        dpi, dv = compare(eng, x[idx], rpi[idx], rv[idx], (kind, n))
        print(f"f16 {kind} n={n}: max |d pi| {dpi:.2e}, max |d v| {dv:.2e}")
    eng.close()
