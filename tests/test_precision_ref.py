"""The CPU model of the NET_BF16 / NET_F16 towers (tests/precision_ref.py) and its exact nets, without a GPU: the model is the plain
float64 graph when rounding is off, its rounding helpers are right, lattice_net passes the exactness certificate at every depth the
GPU tests run, and every rounding-point mistake the GPU tests are meant to catch moves pi or v by 100x their tolerance or more."""
import os

import numpy as np
import pytest
import torch

import azr_testlib as T
import precision_ref as M
import torch_train_ref as R

ELS = [M.BF16, M.F16]


def golden_boards(n):
    g = np.unique(np.load(os.path.join(T.GOLDEN, "encode.npz"))["in88"], axis=0)
    return g[np.linspace(0, len(g) - 1, n).astype(int)].copy()


@pytest.mark.parametrize("blocks", [1, 2])
def test_model_without_rounding_is_the_float64_graph(blocks):
    """rounding off: the model is torch_train_ref.AzrNet in float64 (Glorot weights, perturbed BN), to 1e-12"""
    flat = T.make_net_flat(blocks, seed=3, perturb_bn=True)
    net = R.AzrNet(blocks, flat).double().eval()
    for n in (1, 2, 16):
        x = golden_boards(16)[:n]
        with torch.no_grad():
            lg, rv = net(torch.from_numpy(R.planes_from_in88(x)).double())
        rpi = torch.softmax(lg, 1).numpy()
        pi, v, _ = M.forward(flat, blocks, x, rounding=False)
        assert np.abs(pi - rpi).max() <= 1e-12 and np.abs(v - rv.numpy()).max() <= 1e-12, (n, np.abs(pi - rpi).max())


def test_rounding_helpers():
    """f2bf / f2h of the model bit for bit: NaN, +-0, ties, subnormals, the fp16 overflow; numpy float16 and torch bfloat16 as the
    second opinion on everything else"""
    f32 = lambda *u: np.array(u, np.uint32).view(np.float32)   # noqa: E731
    # bf16: ties to even (1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6), NaN keeps sign and upper payload with the quiet bit
    x = f32(0x3f808000, 0x3f818000, 0x3f808001, 0x80000000, 0x00000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xff812345, 0x7f7fffff)
    want = [0x3f80, 0x3f82, 0x3f81, 0x8000, 0x0000, 0x7f80, 0xff80, 0x7fc0, 0xffc1, 0x7f80]
    assert M.f2bf(x).tolist() == want, [hex(h) for h in M.f2bf(x)]
    # fp16: 65504 = 0x7bff; 65519.99 rounds down, 65520 (the tie above) to inf; 2^-24 the smallest subnormal, 2^-25 a tie to 0,
    # 3 * 2^-25 a tie to 2 * 2^-24; 2048 + 1 a tie to 2048, 2048 + 3 to 2052; NaN quiet with payload
    x = np.array([65504, 65519.99, 65520, 1e6, -65520, 2 ** -24, 2 ** -25, 3 * 2 ** -25, 2049, 2051, -0.0, 0.0, 2 ** -14,
                  2 ** -14 - 2 ** -25, np.inf], np.float32)
    want = [0x7bff, 0x7bff, 0x7c00, 0x7c00, 0xfc00, 0x0001, 0x0000, 0x0002, 0x6800, 0x6802, 0x8000, 0x0000, 0x0400, 0x0400, 0x7c00]
    assert M.f2h(x).tolist() == want, [hex(h) for h in M.f2h(x)]
    assert M.f2h(f32(0x7fc00000, 0xffa00000, 0x7fc02000)).tolist() == [0x7e00, 0xfe00 | 0x100, 0x7e01]
    # the saturating form the kernels store (El<true>::rne, pack_relu): never inf
    assert M.F16.rne(np.array([65520, 1e30, np.inf], np.float32)).tolist() == [65504.0] * 3
    # random values over the whole range, and exact ties of both parities, against numpy / torch
    rng = np.random.default_rng(1)
    u = rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)
    r = u.view(np.float32)
    r = r[np.isfinite(r)]
    ties = np.concatenate([(u[:20000] & 0xffff0000) | 0x8000, (u[:20000] & 0xffffe000) | 0x1000]).astype(np.uint32).view(np.float32)
    scaled = (rng.standard_normal(100000) * np.exp2(rng.integers(-30, 20, 100000))).astype(np.float32)
    for v in (r, ties[np.isfinite(ties)], scaled):
        with np.errstate(over="ignore"):
            want16 = v.astype(np.float16)
        assert (M.f2bf(v) == torch.from_numpy(v).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)).all()
        assert (M.f2h(v) == want16.view(np.uint16)).all()
        assert (M.bf2f(M.f2bf(v)) == torch.from_numpy(v).to(torch.bfloat16).float().numpy()).all()
        assert (M.h2f(M.f2h(v)) == want16.astype(np.float32)).all()
    # toward zero (the truncation variant)
    assert (M.f2bf(scaled, trunc=True) == (scaled.view(np.uint32) >> 16)).all()
    t = M.h2f(M.f2h(scaled, trunc=True)).astype(np.float64)
    fin = np.abs(scaled) < 65504
    assert (np.abs(t[fin]) <= np.abs(scaled[fin])).all() and (np.abs(M.h2f(M.f2h(scaled[fin])) - scaled[fin]) <= np.abs(t[fin] - scaled[fin])).all()


def test_f16_scale():
    """f16_scale of azr_net_bf16.hip: max |2^e w| in [2^13, 2^14), e clamped to [-2, 24], 0 for zeros; out of range refused"""
    assert M.f16_scale(np.float32([1.0, -0.5])) == 13
    assert M.f16_scale(np.float32([0.99])) == 14
    assert M.f16_scale(np.float32([2.0 ** -12])) == 24 and M.f16_scale(np.float32([2.0 ** -10])) == 23
    assert M.f16_scale(np.float32([2.0 ** 15, 1])) == -2 and M.f16_scale(np.float32([65000])) == -2
    assert M.f16_scale(np.zeros(9, np.float32)) == 0
    for bad in (65504.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            M.f16_scale(np.float32([1.0, bad]))


def _layer_report(name, st):
    d, vm = np.array(st["density"]), np.array(st["vmax"])
    r = max(x["ratio"] for x in st["layers"])
    print(f"{name}: {len(d)} layers, largest sum|w||a| / (2^24 quantum) {r:.2e}, non-zero activations per layer "
          f"{d.min():.2f} .. {d.max():.2f}, largest activation {vm.max():.4g}")
    return d, vm, r


@pytest.mark.parametrize("el", ELS, ids=lambda e: e.name)
@pytest.mark.parametrize("blocks", [1, 2, 20])
def test_lattice_net_passes_the_certificate(el, blocks):
    """lattice_net on synthetic lattice boards: every conv of the tower exact in fp32, every epilogue fma and shortcut add exact in
    float64 (one fp32 rounding); at least a fifth of the activations of every layer non-zero.  Also with the stem planes that el
    cannot represent (ties included): the certificate holds behind the stem features' rounding"""
    flat = M.lattice_net(blocks, 5, el)
    for exact in (True, False):
        x = M.lattice_boards(64, 9, el, exact_planes=exact)
        pi, v, st = M.forward(flat, blocks, x, el, certify=True)
        d, vm, r = _layer_report(f"{el.name} B={blocks} {'lattice' if exact else 'non-representable'} planes", st)
        assert len(st["layers"]) == 2 * blocks + 1 and r < 1.0
        assert d.min() >= 0.2, d
        assert np.isfinite(pi).all() and np.isfinite(v).all()
        assert v.std() > 0.005 and pi.max(1).min() < 0.95, (v.std(), pi.max(1).min())   # the outputs tell the boards apart
        if not exact:   # the stem really rounds: features and tie planes differ from the fp32 planes
            planes = R.planes_from_in88(x)
            assert (el.rne(planes) != planes).mean() > 0.05


def test_certificate_refuses_inexact_nets():
    """a Glorot net is not exact: forward(certify=True) raises instead of returning a weaker reference"""
    flat = T.make_net_flat(1, seed=3, perturb_bn=True)
    with pytest.raises(M.NotExact):
        M.forward(flat, 1, golden_boards(4), M.BF16, certify=True)
    p = M.from_flat(2, M.lattice_net(2, 5, M.BF16))
    p["b1a_w"] = np.random.default_rng(0).uniform(-0.05, 0.05, p["b1a_w"].shape).astype(np.float32)   # one dense Glorot-like layer
    with pytest.raises(M.NotExact):
        M.forward(M.to_flat(2, p), 2, M.lattice_boards(16, 9), M.BF16, certify=True)


VARIANTS = {
    "truncation instead of RNE": dict(round_mode="trunc"),
    "shortcut added after the rounding": dict(residual="after"),
    "tap dx = +1 dropped at x = 4": dict(drop_tap=(0, 1, 4)),
    "stem BN indexed by column": dict(stem_bn="col"),
    "f16_scale exponent off by one": dict(f16_exp_delta=1),
}


@pytest.mark.parametrize("el", ELS, ids=lambda e: e.name)
def test_model_variants_are_visible(el):
    """on the GPU tests' lattice net at B = 20, each rounding-point mistake moves pi or v by 100x the GPU tolerance or more"""
    blocks = 20
    flat = M.lattice_net(blocks, 5, el)
    x = M.lattice_boards(64, 9, el)
    pi, v, _ = M.forward(flat, blocks, x, el, certify=True)
    for name, kw in VARIANTS.items():
        if "f16_exp_delta" in kw and el is not M.F16:
            continue
        p2, v2, _ = M.forward(flat, blocks, x, el, **kw)
        d = max(np.abs(p2 - pi).max(), np.abs(v2 - v).max())
        print(f"{el.name} B=20 {name:36s}: max |d pi|, |d v| = {d:.2e} = {d / M.GPU_TOL:.0f} x the GPU tolerance")
        assert d >= 100 * M.GPU_TOL, (name, d)


@pytest.mark.parametrize("el", ELS, ids=lambda e: e.name)
def test_one_ulp_of_one_activation_reaches_the_outputs(el):
    """the heads of lattice_net see every tower activation: one ulp up on any sampled non-zero activation of the B = 20 tower output
    moves pi or v (no ReLU of the heads hides it).  One ulp of ONE activation is near the fp32 head noise (median measured: 2e-6 bf16,
    3e-7 f16, against GPU_TOL = 5e-6); the rounding-point mistakes above move thousands of activations and show 100x above it"""
    blocks = 20
    flat = M.lattice_net(blocks, 5, el)
    x = M.lattice_boards(32, 9, el)
    pi, v, _, h = M.forward(flat, blocks, x, el, return_tower=True)
    P = M.from_flat(blocks, flat)
    rng = np.random.default_rng(0)
    nz = np.argwhere(h > 0)
    eff = []
    for i in rng.choice(len(nz), 200, replace=False):
        idx = tuple(nz[i])
        h2 = h[idx[0]:idx[0] + 1].copy()
        bits = el.to_bits(np.float32([h[idx]]))[0]
        h2[(0,) + idx[1:]] = el.to_f(np.array([bits + 1], np.uint16))[0]
        p2, v2 = M.heads(P, h2)
        eff.append(max(np.abs(p2[0] - pi[idx[0]]).max(), abs(v2[0] - v[idx[0]])))
    eff = np.array(eff)
    q = np.quantile(eff, [0.1, 0.5, 0.9])
    print(f"{el.name}: one ulp of one activation moves pi / v by {q[0]:.1e} / {q[1]:.1e} / {q[2]:.1e} (10 / 50 / 90 %)")
    assert eff.min() > 1e-12
    assert np.median(eff) >= M.GPU_TOL / (4 if el is M.BF16 else 40), q


def test_f16_edge_nets_pass_the_certificate():
    """the NET_F16 edge nets of tests/test_gpu_net_exact.py: exact, and they reach the edges they are named after"""
    x = M.lattice_boards(64, 9, M.F16)
    _, _, st = M.forward(M.f16_edge_net("scale_clamps", 5), 2, x, M.F16, certify=True)
    assert st["exps"] == [13, 24, -2, 0, 13], st["exps"]
    _, _, st, h = M.forward(M.f16_edge_net("saturation", 5), 2, x, M.F16, certify=True, return_tower=True)
    top = h[h >= 32768]
    print("saturation: tower outputs >= 32768:", np.unique(top)[:8], "... share at 65504: %.3f" % (top == 65504).mean())
    assert (top == 65504).any() and (top < 65504).any() and np.isfinite(h).all()
    _, _, st, h = M.forward(M.f16_edge_net("subnormal", 5), 2, x, M.F16, certify=True, return_tower=True)
    sub = (h > 0) & (h < 2.0 ** -14)
    print("subnormal: share of fp16 subnormals among the non-zero tower outputs %.2f" % (sub.sum() / (h > 0).sum()))
    assert sub.sum() >= 0.5 * (h > 0).sum()


# ---------------------------------------------------------------------------------------------------------------------------------
# NET_F32X: the fp16-pair element (precision_ref.forward_fx, lattice_net_fx)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_pair_split_properties():
    """hi = rne16(x), lo = rne16(x - hi) on random fp32 values over the fp16 range: hi + lo is exact in fp32; the pair is within
    2^-22 |x| of x where lo is a normal fp16 number and within 2^-25 absolute where it is subnormal (or zero)"""
    rng = np.random.default_rng(2)
    x = (rng.standard_normal(400000) * np.exp2(rng.integers(-30, 15, 400000))).astype(np.float32)
    x = x[np.abs(x) < 65504]
    hi, lo = M.split_pair(x)
    s64 = hi.astype(np.float64) + lo.astype(np.float64)
    assert ((hi + lo).astype(np.float64) == s64).all()
    err = np.abs(x.astype(np.float64) - s64)
    normal = np.abs(lo) >= 2.0 ** -14
    assert normal.sum() > 50000 and (~normal).sum() > 50000
    assert (err[normal] <= 2.0 ** -22 * np.abs(x[normal]).astype(np.float64)).all()
    assert (err[~normal] <= 2.0 ** -25).all()
    assert (M.h2f(M.f2h(hi)) == hi).all() and (M.h2f(M.f2h(lo)) == lo).all()
    sub = (lo != 0) & ~normal
    assert sub.sum() > 10000 and (np.abs(lo[sub]) >= 2.0 ** -24).all()      # subnormal low parts keep their value


@pytest.mark.parametrize("blocks", [1, 2])
def test_pair_model_without_rounding_is_the_float64_graph(blocks):
    flat = T.make_net_flat(blocks, seed=3, perturb_bn=True)
    net = R.AzrNet(blocks, flat).double().eval()
    x = golden_boards(16)
    with torch.no_grad():
        lg, rv = net(torch.from_numpy(R.planes_from_in88(x)).double())
    rpi = torch.softmax(lg, 1).numpy()
    pi, v, _ = M.forward_fx(flat, blocks, x, rounding=False)
    assert np.abs(pi - rpi).max() <= 1e-12 and np.abs(v - rv.numpy()).max() <= 1e-12, np.abs(pi - rpi).max()


def test_pair_model_on_a_dense_net():
    """an ordinary dense net (Glorot weights, perturbed BN) at B = 2: the pair model is within 1e-5 of the plain float64 graph (a
    sanity bound, not a claim: the kernel's own figure is 3e-6 at B = 20)"""
    flat = T.make_net_flat(2, seed=3, perturb_bn=True)
    x = golden_boards(16)
    rpi, rv, _ = M.forward_fx(flat, 2, x, rounding=False)
    pi, v, st = M.forward_fx(flat, 2, x)
    d = max(np.abs(pi - rpi).max(), np.abs(v - rv).max())
    print(f"pair model vs float64 graph, dense B=2: {d:.2e}; layer exponents {st['exps']}")
    assert d <= 1e-5, d
    p2, v2, _ = M.forward_fx(flat, 2, x, variant=dict(kind="with_al_wl"))
    assert max(np.abs(p2 - rpi).max(), np.abs(v2 - rv).max()) <= 1e-5


@pytest.mark.parametrize("blocks", [1, 2, 20])
def test_fx_lattice_net_passes_the_certificate(blocks):
    """lattice_net_fx on the whole pool of the GPU test: every output's terms (ah wh, al wh, ah wl) on one quantum with
    sum |term| < 2^24 of it, every fma and shortcut add exact in float64"""
    flat, x, pi, v, st = M.fx_pool(blocks)
    r = max(l["ratio"] for l in st["layers"])
    print(f"f32x B={blocks}: largest sum |term| / (2^24 quantum) {r:.2f}, largest activation {max(st['vmax']):.4g}, "
          f"layer exponents {sorted(set(st['exps']))}")
    assert len(st["layers"]) == 2 * blocks + 1 and 0 < r < 1.0
    assert set(st["exps"]) == {13}
    assert np.isfinite(pi).all() and np.isfinite(v).all()
    assert v.std() > 0.005 and pi.max(1).min() < 0.95, (v.std(), pi.max(1).min())


def test_fx_certificate_refuses_inexact_nets():
    """one rich weight reading a rich channel (both low parts non-zero: 12 + 12 significand bits and a sum) breaks the certificate;
    so does a dense Glorot net"""
    blocks = 2
    x = M.fx_boards(16, 9)
    p = M.from_flat(blocks, M.lattice_net_fx(blocks, 5))
    M.forward_fx(M.to_flat(blocks, p), blocks, x, certify=True)
    W = p["b1a_w"]
    ci, co = 33, 37                                            # rich input channel, rich output channel
    rich_w = W[W != np.round(W)].ravel()[0]
    ky, kx = [(a, b) for a in range(3) for b in range(3) if W[a, b, ci, co] == 0][0]
    W[ky, kx, ci, co] = rich_w
    with pytest.raises(M.NotExact):
        M.forward_fx(M.to_flat(blocks, p), blocks, x, certify=True)
    with pytest.raises(M.NotExact):
        M.forward_fx(T.make_net_flat(1, seed=3, perturb_bn=True), 1, golden_boards(2), certify=True)


def test_fx_lattice_net_is_not_vacuous():
    """the B = 20 net on the pool of the GPU test: every fragment position (tap, k-slice, column tile) of the layer loop meets, in
    some layer, a rich weight (wl != 0) on a non-zero ah and a ternary weight on an activation with al != 0 — for every tap both in a
    border cell and in an interior cell of the board; in every layer at least 10 % of the non-zero activations entering the
    rich-reading weights have al != 0, at least 25 % of the outputs are non-zero and at least 10 % are zero"""
    blocks = 20
    flat, x, pi, v, st = M.fx_pool(blocks)
    cov = st["coverage"]
    assert len(x) == 256 and len(cov) == 2 * blocks
    for kind in ("rich", "tern"):
        live = np.any([c[kind] for c in cov], 0)
        assert live.shape == (9, 8, 16) and live.all(), (kind, np.argwhere(~live))
        cells = np.any([c["cell_" + kind] for c in cov], 0)
        assert cells.shape == (9, 2) and cells.all(), (kind, cells)
    share = np.array([c["enter_lo"] / c["enter"] for c in cov])
    d = np.array(st["density"])
    print(f"f32x B=20: al != 0 on {share.min():.2f} .. {share.max():.2f} of the activations entering rich-reading weights, "
          f"non-zero outputs per layer {d.min():.2f} .. {d.max():.2f}")
    assert share.min() >= 0.10 and d.min() >= 0.25 and d.max() <= 0.90, (share.min(), d.min(), d.max())
    # the term the kernel leaves out is identically zero on this net: no weight with wl != 0 reads an activation with al != 0
    p2, v2, _ = M.forward_fx(flat, blocks, x[:8], variant=dict(kind="with_al_wl"))
    assert (p2 == pi[:8]).all() and (v2 == v[:8]).all()


def test_fx_model_variants_are_visible():
    """what the GPU test would see: each mistake of the layer loop, confined to ONE layer, tap, k-slice and column tile — in the first,
    a middle and the last conv layer, at the busiest live position of the coverage table — moves pi or v of some board of the pool
    by 4 x GPU_TOL or more; so does a shortcut taken from the pair instead of the fp32 registers (anywhere).  (al wl included is
    not among them: on the lattice net that term is zero — test_fx_lattice_net_is_not_vacuous.)"""
    blocks = 20
    flat, x, pi, v, st = M.fx_pool(blocks)
    cov = st["coverage"]
    sub = slice(0, 96)
    for L in (0, blocks, 2 * blocks - 1):
        rich_pos = np.unravel_index(np.argmax(cov[L]["rich_n"]), (9, 8, 16))
        tern_pos = np.unravel_index(np.argmax(cov[L]["tern_n"] * (np.arange(8) >= 1)[None, :, None]), (9, 8, 16))   # stale_al: ks >= 1
        for kind, pos in (("drop_wh_al", tern_pos), ("drop_wl_ah", rich_pos), ("wl_ah_next_tile", rich_pos), ("stale_al", tern_pos)):
            assert cov[L]["rich" if pos is rich_pos else "tern"][pos]
            var = dict(kind=kind, layer=L, tap=int(pos[0]), ks=int(pos[1]), ct=int(pos[2]))
            p2, v2, _ = M.forward_fx(flat, blocks, x[sub], variant=var)
            d = max(np.abs(p2 - pi[sub]).max(), np.abs(v2 - v[sub]).max())
            print(f"f32x B=20 layer {L:2d} {kind:16s} at (tap, ks, ct) = {tuple(int(i) for i in pos)}: {d:.2e} = {d / M.GPU_TOL:.0f} x GPU_TOL")
            assert d >= 4 * M.GPU_TOL, (var, d)
    p2, v2, _ = M.forward_fx(flat, blocks, x[sub], variant=dict(kind="shortcut_pair"))
    d = max(np.abs(p2 - pi[sub]).max(), np.abs(v2 - v[sub]).max())
    print(f"f32x B=20 shortcut taken from hi + lo: {d:.2e} = {d / M.GPU_TOL:.0f} x GPU_TOL")
    assert d >= 4 * M.GPU_TOL, d


def test_fx_edge_and_stem_nets_pass_the_certificate():
    """the nets of the GPU tests at the edges of the layer scale reach them, exactly; and the stem keeps planes that fp16 cannot
    represent: the certificate holds on them in fp32, and rounding them to fp16 first would move the outputs"""
    x = M.fx_boards(64, 11)
    _, _, st = M.forward_fx(M.fx_edge_net("scale_clamps", 5), 2, x, certify=True)
    assert st["exps"] == [24, -2, 0, 13], st["exps"]
    flat = M.fx_edge_net("subnormal_wl", 5)
    _, _, st = M.forward_fx(flat, 2, x, certify=True, coverage=True)
    assert st["exps"] == [13] * 4
    _, wl = M.split_pair(M.from_flat(2, flat)["b1b_w"] * np.float32(2.0 ** 13))
    sub = (wl != 0) & (np.abs(wl) < 2.0 ** -14)
    assert sub.sum() == 21 and st["coverage"][3]["rich"][:, :, 5].any()      # 7 rich channels x 3 rich weights, live
    xs = M.fx_boards(96, 10, exact_planes=False)
    planes = R.planes_from_in88(xs)
    assert (M.F16.rne(planes) != planes).mean() > 0.05
    flat = M.lattice_net_fx(2, 6, stem_fine=0)
    pi, v, _ = M.forward_fx(flat, 2, xs, certify=True)
    f = xs[:, 48:88].copy().view(np.float32).reshape(-1, 10)
    xr = xs.copy()
    xr[:, 48:88] = M.F16.rne(f).view(np.uint8).reshape(-1, 40)
    p2, v2, _ = M.forward_fx(flat, 2, xr)
    d = max(np.abs(p2 - pi).max(), np.abs(v2 - v).max())
    print(f"stem planes rounded to fp16 first: {d:.2e} = {d / M.GPU_TOL:.0f} x GPU_TOL")
    assert d >= 4 * M.GPU_TOL
