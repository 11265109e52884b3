"""CPU model of the reduced-precision towers NET_BF16 / NET_F16 (TEST INFRASTRUCTURE, not a conftest).

It follows csrc/azr_net_bf16.hip and csrc/azr_bf16_common.hpp step by step, on the CPU, in float64 with the kernels'
rounding points made explicit:
  * stem planes: plane_value (tests/torch_train_ref.planes_from_in88), then El<F16>::rne (fp16 clamps at 65504 first);
  * weights: f2bf(w), or f2h(w * 2^e) with e from f16_scale and 2^-e folded into the layer's BN scale;
  * fold: fold_bn in fp32 (s = g / sqrtf(v + 1e-3f), shift = b - m * s, no contraction), the stem's BN indexed by the board row;
  * epilogue: fmaf(acc, s, shift) (one rounding), on the second conv of a block + the 16-bit block input in fp32 (one rounding),
    ReLU, round to nearest even; fp16 saturates at 0x7bff (pack_relu);
  * heads: float64 on the tower output.

The conv accumulation is done in float64.  On a net whose arithmetic is exact — every product and every partial sum a multiple of
one quantum and below 2^24 of it — any summation order gives the same fp32 sum, so the towers' output is one well-defined set of
bits whatever the MFMA order.  `forward(..., certify=True)` checks that per layer (the exactness certificate) and raises otherwise;
`lattice_net` builds nets that pass it."""
import numpy as np
import torch

import torch_train_ref as R

F_ = 256
BN_EPS32 = np.float32(1e-3)
# var such that float32(var) + float32(1e-3) == 1.0 exactly: the folded BN scale is then exactly gamma
VAR_ONE = np.float32(1.0) - BN_EPS32
assert VAR_ONE + BN_EPS32 == np.float32(1.0)

# GPU tolerance of tests/test_gpu_net_exact.py on pi and v against this model: fp32 head noise only (the tower is exact; measured
# on the MI355X: 2.3e-6 on pi, 3.4e-7 on v)
GPU_TOL = 5e-6


# ---------------------------------------------------------------------------------------------------------------------------------
# rounding helpers: float32 arrays -> 16-bit patterns, and back
# ---------------------------------------------------------------------------------------------------------------------------------
def f2bf(x, trunc=False):
    """azr_bf16_common.hpp f2bf (= the kernels' v_cvt_pk_bf16_f32 on non-NaN values): round to nearest even; NaN stays NaN
    (quiet bit set, sign and upper payload kept).  trunc: toward zero instead (a model variant, not the kernels)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7fffffff) > 0x7f800000
    r = (u >> 16) if trunc else ((u + 0x7fff + ((u >> 16) & 1)) >> 16)
    r = np.where(nan, (u >> 16) | 0x40, r)
    return (r & 0xffff).astype(np.uint16)


def bf2f(h):
    return (np.asarray(h, np.uint16).astype(np.uint32) << 16).view(np.float32)


def f2h(x, trunc=False):
    """float32 -> fp16 bits as `(_Float16)f` converts (host f2h of azr_net_bf16.hip, device v_cvt_f16_f32): round to nearest even,
    subnormals kept, overflow to inf, NaN quiet with the upper payload bits.  trunc: toward zero (a model variant)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.int64)
    sign = (u >> 16) & 0x8000
    a = u & 0x7fffffff
    e = a >> 23
    m = (a & 0x7fffff) | 0x800000
    # normal results (|x| >= 2^-14): keep 10 fraction bits; subnormal results: units of 2^-24
    s = np.where(a >= 0x38800000, 13, np.clip(126 - e, 14, 40))
    base = np.where(a >= 0x38800000, ((e - 112) << 10) + ((a & 0x7fffff) >> 13), m >> s)
    rem = m & ((np.int64(1) << s) - 1)
    half = np.int64(1) << (s - 1)
    up = (rem > half) | ((rem == half) & ((base & 1) == 1))
    h = base + (0 if trunc else up)
    h = np.where(e == 0, 0, h)                                           # float32 zero / subnormal: below half of 2^-24
    h = np.where(a >= (0x477fe000 if trunc else 0x477ff000), 0x7bff if trunc else 0x7c00, h)   # >= 65520 rounds to inf
    h = np.where(a == 0x7f800000, 0x7c00, h)
    h = np.where(a > 0x7f800000, 0x7e00 | ((a >> 13) & 0x1ff), h)
    return (sign | h).astype(np.uint16)


def h2f(h):
    return np.asarray(h, np.uint16).view(np.float16).astype(np.float32)


class Elem:
    """the 16-bit element type of a tower (El<false> / El<true>); q = the quantum of lattice_net's activations"""

    def __init__(self, name, to_bits, to_f, q):
        self.name, self.to_bits, self.to_f, self.q = name, to_bits, to_f, q

    def rne(self, x, trunc=False):
        """El<F16>::rne / pack_relu on float32 values -> float32 values of the rounded elements (fp16: saturated at 65504, as
        fminf before the conversion and the integer min with 0x7bff after it both do)"""
        x = np.asarray(x, np.float32)
        if self.name == "f16":
            x = np.minimum(x, np.float32(65504.0))
        return self.to_f(self.to_bits(x, trunc=trunc))


BF16 = Elem("bf16", f2bf, bf2f, 2.0 ** -8)
F16 = Elem("f16", f2h, h2f, 2.0 ** -11)
ELEMS = {"bf16": BF16, "f16": F16}


def f16_scale(W):
    """azr_net_bf16.hip f16_scale: e such that max |2^e w| is in [2^13, 2^14), clamped to [-2, 24]; 0 for an all-zero tensor"""
    worst = np.float32(np.abs(np.asarray(W, np.float32)).max())
    if not worst < np.float32(65504.0):
        raise ValueError("NET_F16: a weight is outside the fp16 range or not a number")
    if worst == 0:
        return 0
    we = int(np.frexp(worst)[1])
    return int(min(24, max(-2, 14 - we)))


# ---------------------------------------------------------------------------------------------------------------------------------
# the exactness certificate
# ---------------------------------------------------------------------------------------------------------------------------------
def quantum(x):
    """largest power of two dividing every non-zero entry of the float64 array x (inf if there is none)"""
    x = np.abs(np.asarray(x, np.float64).ravel())
    x = x[x != 0]
    if x.size == 0:
        return np.inf
    m, e = np.frexp(x)
    mi = (m * 2.0 ** 53).astype(np.int64)
    return float(np.min(np.ldexp((mi & -mi).astype(np.float64), e - 53)))


def two_sum_exact(a, b):
    """True where a + b is exact in float64 (the TwoSum error term is zero)"""
    s = a + b
    bb = s - a
    err = (a - (s - bb)) + (b - bb)
    return err == 0


class NotExact(AssertionError):
    pass


# ---------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------
def _params(flat, blocks):
    lay, count = R.layout(blocks)
    flat = np.asarray(flat, np.float32)
    assert flat.size == count
    return {name: flat[off:off + int(np.prod(shape))].reshape(shape) for name, off, shape in lay}


def fold_bn32(bn):
    """azr_net.hip fold_bn: fp32, -ffp-contract=off"""
    g, b, m, v = (np.asarray(bn[i], np.float32) for i in range(4))
    s = g / np.sqrt(v + BN_EPS32)
    return s, b - m * s


def _pad(a):   # [n, 7, 6, C] -> [n, 9, 8, C] with a zero border
    return torch.nn.functional.pad(a, (0, 0, 1, 1, 1, 1))


def conv3x3(a, W, dtype=torch.float64, drop=None):
    """3x3 SAME conv of [n, 7, 6, Cin] with HWIO weights W [3, 3, Cin, Cout] (numpy), accumulated in `dtype`.  Sparse weights
    (the lattice nets) go through index_add over their non-zeros.  drop = (dy, dx, x): the tap (dy, dx) is left out for the
    output cells of column x (a model variant: a border mask in the wrong place)"""
    n = a.shape[0]
    cout = W.shape[3]
    ap = _pad(a.to(dtype))
    Wt = torch.from_numpy(np.asarray(W, np.float64)).to(dtype)
    out = torch.zeros(n, 7, 6, cout, dtype=dtype)
    sparse = np.count_nonzero(W) <= 0.05 * W.size
    for ky in range(3):
        for kx in range(3):
            S = ap[:, ky:ky + 7, kx:kx + 6, :]
            if sparse:
                ci, co = torch.nonzero(Wt[ky, kx], as_tuple=True)
                if len(ci) == 0:
                    continue
                P = S[..., ci] * Wt[ky, kx, ci, co]
            else:
                P = S @ Wt[ky, kx]
            if drop is not None and (ky - 1, kx - 1) == tuple(drop[:2]):
                P = P.clone()
                P[:, :, drop[2], :] = 0
            if sparse:
                out.index_add_(3, co, P)
            else:
                out += P
    return out


def _certify_conv(tag, a, W, acc, stats):
    """every product a multiple of q = quantum(W) * quantum(a) and sum |w| |a| < 2^24 q for every output: then every partial sum
    of every order is an exact fp32 number, and acc (float64) is THE fp32 sum"""
    qw, qa = quantum(W), quantum(a.numpy())
    if not np.isfinite(qw) or not np.isfinite(qa):
        stats.append(dict(layer=tag, ratio=0.0))
        return
    q = qw * qa
    bound = conv3x3(a.abs(), np.abs(W)).max().item()
    ratio = bound / (2.0 ** 24 * q)
    stats.append(dict(layer=tag, ratio=ratio, q=q))
    if not (ratio < 1.0 and q >= 2.0 ** -149):
        raise NotExact(f"{tag}: sum |w||a| = {bound:.6g} is not below 2^24 x quantum {q:.3g} (ratio {ratio:.3g})")
    assert torch.equal(acc, acc.to(torch.float32).to(torch.float64)), tag


def forward(flat, blocks, in88, el=BF16, rounding=True, certify=False, accum="f64", round_mode="rne", residual="before",
            drop_tap=None, stem_bn="row", f16_exp_delta=0, return_tower=False):
    """pi [n, 43], v [n] (float64) of NET_BF16 (el = BF16) or NET_F16 (el = F16) on the boards in88 [n, 88].
    rounding=False: the plain float64 graph (= torch_train_ref.AzrNet).  accum: "f64" (exact on certified nets) or "f32".
    Model variants (none of them is what the kernels do; the tests show that each one is visible): round_mode "trunc",
    residual "after" (added to the ROUNDED conv output, then rounded again), drop_tap (dy, dx, x), stem_bn "col",
    f16_exp_delta (the packing exponent off, the fold's 2^-e not)."""
    p = _params(flat, blocks)
    n = len(in88)
    cdt = torch.float64 if accum == "f64" else torch.float32
    trunc = round_mode == "trunc"
    stats = dict(layers=[], density=[], vmax=[], exps=[])

    def pack(W):
        W = np.asarray(W, np.float32)
        if not rounding:
            return W.astype(np.float64), 1.0
        if el is BF16:
            return bf2f(f2bf(W)).astype(np.float64), np.float32(1.0)
        e = f16_scale(W)
        stats["exps"].append(e)
        return h2f(f2h(W * np.float32(2.0 ** (e + f16_exp_delta)))).astype(np.float64), np.float32(2.0 ** -e)

    def fold(bn, unscale):
        if not rounding:
            g, b, m, v = (np.asarray(bn[i], np.float64) for i in range(4))
            s = g / np.sqrt(v + 1e-3)
            return s, b - m * s
        s, sh = fold_bn32(bn)
        return (s * unscale).astype(np.float32), sh

    def epilogue(tag, acc, s, sh, res=None):
        """acc [n, 7, 6, C]; s, sh broadcastable (per channel, or per board row / column for the stem)"""
        acc = acc.numpy().astype(np.float64)
        if not rounding:
            v = acc * s + sh + (0.0 if res is None else res)
            return np.maximum(v, 0.0)
        s64, sh64 = np.asarray(s, np.float64), np.asarray(sh, np.float32).astype(np.float64)
        t = acc * s64                                   # exact: 24 x 24 significand bits
        if certify and not two_sum_exact(t, np.broadcast_to(sh64, t.shape)).all():
            raise NotExact(f"{tag}: fmaf(acc, s, shift) is not exact in float64")
        v = (t + sh64).astype(np.float32)               # = fmaf(acc, s, shift): one rounding of the exact value
        if res is not None:
            if residual == "after":
                v = el.rne(v, trunc)
            r64 = v.astype(np.float64)
            if certify and not two_sum_exact(r64, res).all():
                raise NotExact(f"{tag}: the shortcut add is not exact in float64")
            v = (r64 + res).astype(np.float32)          # fp32 add: one rounding
        out = el.rne(np.maximum(v, np.float32(0)), trunc).astype(np.float64)
        valid = out.reshape(-1, out.shape[-1])
        stats["density"].append(float(np.count_nonzero(valid)) / valid.size)
        stats["vmax"].append(float(valid.max()))
        return out

    # stem
    x = np.ascontiguousarray(R.planes_from_in88(in88).transpose(0, 2, 3, 1))   # [n, 7, 6, 13]
    if rounding:
        x = el.rne(x).astype(np.float64)
    a = torch.from_numpy(x.astype(np.float64))
    W, unscale = pack(p["stem_w"])
    acc = conv3x3(a, W, cdt, drop_tap)
    if certify:
        _certify_conv("stem", a, W, acc, stats["layers"])
    s, sh = fold(p["stem_bn"], unscale)                 # 7 per board row
    if stem_bn == "col":                                 # variant: indexed by the column (x = 0..5) instead
        s, sh = s[:6].reshape(1, 1, 6, 1), sh[:6].reshape(1, 1, 6, 1)
    else:
        s, sh = s.reshape(1, 7, 1, 1), sh.reshape(1, 7, 1, 1)
    h = epilogue("stem", acc, s, sh)
    # tower
    for b in range(blocks):
        res = h
        for ab in "ab":
            W, unscale = pack(p[f"b{b}{ab}_w"])
            a = torch.from_numpy(h)
            acc = conv3x3(a, W, cdt, drop_tap)
            if certify:
                _certify_conv(f"b{b}{ab}", a, W, acc, stats["layers"])
            s, sh = fold(p[f"b{b}{ab}_bn"], unscale)
            h = epilogue(f"b{b}{ab}", acc, s, sh, res if ab == "b" else None)
    pi, v = heads(p, h)
    if return_tower:
        return pi, v, stats, h
    return pi, v, stats


def heads(p, h):
    """both heads in float64 on the tower output h [n, 7, 6, 256] (build_graph.py:76-90, torch_train_ref.AzrNet)"""
    n = h.shape[0]
    h = h.reshape(n, 42, F_)

    def bn(x, prm):
        g, b, m, v = (np.asarray(prm[i], np.float64) for i in range(4))
        return (x - m) * (g / np.sqrt(v + 1e-3)) + b

    f = np.maximum(bn(h @ p["pi_w"].astype(np.float64), p["pi_bn"]), 0).reshape(n, 84)
    lg = f @ p["pd_w"].astype(np.float64) + p["pd_b"].astype(np.float64)
    lg -= lg.max(1, keepdims=True)
    pi = np.exp(lg)
    pi /= pi.sum(1, keepdims=True)
    fv = np.maximum(bn(h @ p["v_w"].astype(np.float64), p["v_bn"]), 0).reshape(n, 42)
    hid = np.maximum(fv @ p["v1_w"].astype(np.float64) + p["v1_b"].astype(np.float64), 0)
    v = np.tanh(hid @ p["v2_w"].astype(np.float64)[:, 0] + float(p["v2_b"][0]))
    return pi, v


# ---------------------------------------------------------------------------------------------------------------------------------
# exact nets and boards
# ---------------------------------------------------------------------------------------------------------------------------------
def _sparse_ternary(rng, cin, nnz, balanced=False):
    """[3, 3, Cin, 256] float32 with `nnz` entries of +-1 in every output channel, spread over all taps and input channels;
    balanced: as many +1 as -1 in every channel"""
    W = np.zeros((9 * cin, F_), np.float32)
    for co in range(F_):
        idx = rng.choice(9 * cin, nnz, replace=False)
        W[idx, co] = rng.permutation(np.arange(nnz) % 2 * 2 - 1) if balanced else rng.choice(np.array([-1.0, 1.0], np.float32), nnz)
    return W.reshape(3, 3, cin, F_)


def _multiples(rng, lo, hi, q, size):
    return (np.round(rng.uniform(lo, hi, size) / q) * q).astype(np.float32)


def lattice_net(blocks, seed, el=BF16, nnz=2, stem_nnz=6, beta=(-0.75, 0.25), beta_b=(-1.5, 0.0), balanced=True, head_gain=None):
    """an AZRW flat vector whose NET_BF16 / NET_F16 arithmetic is exact on lattice boards (certificate of forward()): conv
    weights sparse ternary (nnz per output channel), every BN folds to scale 1 (gamma 1, mean 0, var + 1e-3 == 1 in fp32) with a
    shift on the quantum el.q (the first conv of a block in `beta`, the second in `beta_b`: mostly negative, so ReLU zeroes part of
    every layer); the stem's seven row shifts differ.  Heads: dense, logits O(1) and a value pre-activation O(0.5), so that one ulp
    of one tower activation shows in pi or v far above the fp32 head noise"""
    rng = np.random.default_rng(seed)
    q = el.q
    out = {}
    out["stem_w"] = _sparse_ternary(rng, 13, stem_nnz)
    stem_b = rng.permutation(np.arange(-3, 4)).astype(np.float32) * np.float32(8 * q) + np.float32(0.25)
    out["stem_bn"] = np.stack([np.ones(7, np.float32), stem_b, np.zeros(7, np.float32), np.full(7, VAR_ONE)])
    for b in range(blocks):
        for ab, (lo, hi) in (("a", beta), ("b", beta_b)):
            out[f"b{b}{ab}_w"] = _sparse_ternary(rng, F_, nnz, balanced and ab == "b")
            out[f"b{b}{ab}_bn"] = np.stack([np.ones(F_, np.float32), _multiples(rng, lo, hi, q, F_),
                                            np.zeros(F_, np.float32), np.full(F_, VAR_ONE)])
    g = np.float32(1.25 ** blocks if head_gain is None else head_gain)   # the activations grow by about 1.25 per block
    out["pi_w"] = rng.uniform(-1, 1, (F_, 2)).astype(np.float32) * np.float32(0.05) / g
    out["pi_bn"] = np.stack([np.ones(2), np.full(2, 2.0), np.zeros(2), np.ones(2)]).astype(np.float32)
    out["pd_w"] = rng.uniform(-0.5, 0.5, (84, 43)).astype(np.float32)
    out["pd_b"] = rng.uniform(-0.2, 0.2, 43).astype(np.float32)
    out["v_w"] = rng.uniform(-1, 1, (F_, 1)).astype(np.float32) * np.float32(0.05) / g
    out["v_bn"] = np.array([[1.0], [2.0], [0.0], [1.0]], np.float32)
    out["v1_w"] = rng.uniform(-0.3, 0.3, (42, 256)).astype(np.float32)
    out["v1_b"] = rng.uniform(-0.1, 0.3, 256).astype(np.float32)
    out["v2_w"] = rng.uniform(-0.05, 0.05, (256, 1)).astype(np.float32)
    out["v2_b"] = np.array([0.1], np.float32)
    return to_flat(blocks, out)


def to_flat(blocks, params):
    lay, count = R.layout(blocks)
    flat = np.zeros(count, np.float32)
    for name, off, shape in lay:
        flat[off:off + int(np.prod(shape))] = np.asarray(params[name], np.float32).reshape(-1)
    return flat


def from_flat(blocks, flat):
    return {k: v.copy() for k, v in _params(flat, blocks).items()}


def f16_edge_net(kind, seed):
    """two-block NET_F16 nets at the edges of the fp16 range, exact like lattice_net:
      "scale_clamps": the first conv's weights are +-2^-12 (f16_scale: e = 14 + 11 = 25 -> clamped to 24) with gamma 2^12, the
                      second's +-2^15 (e = -2) with gamma 2^-15, the third conv all zeros (e = 0)
      "saturation":   the shifts of 24 channels of the first block's second conv drive them across 65504 (65000 .. 70000 and 1e6),
                      the second block reads none of them but carries them on its shortcut; the heads see them at +-2^-16
      "subnormal":    the stem's gamma is 2^-20 (shifts on 2^-24): the tower runs on fp16 subnormals; heads scaled by 2^14"""
    blocks = 2
    if kind == "subnormal":
        p = from_flat(blocks, lattice_net(blocks, seed, F16, head_gain=2.0 ** -14))
        rng = np.random.default_rng(seed + 7)
        p["stem_bn"][0] = np.float32(2.0 ** -20)
        p["stem_bn"][1] = rng.permutation(np.arange(-3, 4)).astype(np.float32) * np.float32(2.0 ** -22) + np.float32(2.0 ** -19)
        for b in range(blocks):
            for ab in "ab":
                p[f"b{b}{ab}_bn"][1] = _multiples(rng, -2.0 ** -18, 2.0 ** -19, 2.0 ** -24, F_)
        return to_flat(blocks, p)
    p = from_flat(blocks, lattice_net(blocks, seed, F16))
    if kind == "scale_clamps":
        p["b0a_w"] *= np.float32(2.0 ** -12)
        p["b0a_bn"][0] = np.float32(2.0 ** 12)
        p["b0b_w"] *= np.float32(2.0 ** 15)
        p["b0b_bn"][0] = np.float32(2.0 ** -15)
        p["b1a_w"][:] = 0
        p["b1a_bn"][1] = np.abs(p["b1a_bn"][1])
        return to_flat(blocks, p)
    assert kind == "saturation", kind
    rng = np.random.default_rng(seed + 11)
    sat = rng.choice(F_, 24, replace=False)
    p["b0b_bn"][1][sat] = np.concatenate([np.float32([65504, 65500, 65510, 65520, 65530, 70000, 1e6]),
                                          _multiples(rng, 65000, 66000, 2.0 ** -3, 17)])
    for ab in "ab":
        p[f"b1{ab}_w"][:, :, sat, :] = 0
    sign = np.where(np.arange(24) % 2 == 0, 1.0, -1.0).astype(np.float32)   # opposite signs: the heads see the differences
    p["pi_w"][sat] = (sign * np.float32(2.0 ** -16))[:, None] * np.float32([1, -1])
    p["v_w"][sat] = (sign * np.float32(-2.0 ** -16))[:, None]
    return to_flat(blocks, p)


def lattice_boards(n, seed, el=BF16, exact_planes=True):
    """n distinct NNInputData images: owners 0..2, armies 0..63, current player 0 / 1, and the ten float planes on the quantum
    el.q in [0, 1] (exact_planes) — or (exact_planes=False) float32 values in [1/4, 1] that el cannot represent, a third of them
    exact ties between two neighbours of el (both parities), plus zeros: they exercise the stem features' rounding"""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 88), np.uint8)
    x[:, :42] = (rng.integers(0, 3, (n, 42)) << 6) | rng.integers(0, 64, (n, 42))
    x[:, 42] = rng.integers(0, 2, n)
    if exact_planes:
        f = (rng.integers(0, int(1 / el.q) + 1, (n, 10)) * el.q).astype(np.float32)
    else:
        f = rng.uniform(0.25, 1.0, (n, 10)).astype(np.float32)
        # el's neighbours of f: a tie is their midpoint (an fp32 number: 8 or 11 significand bits + 1)
        lo = el.to_f(el.to_bits(f, trunc=True)).astype(np.float64)
        ulp = np.where(lo < 0.5, 0.25, 0.5) * (2.0 ** -7 if el is BF16 else 2.0 ** -10)
        tie = rng.random((n, 10)) < 1 / 3
        f = np.where(tie, (lo + ulp / 2).astype(np.float32), f)
        f[rng.random((n, 10)) < 0.1] = 0
    x[:, 48:88] = f.view(np.uint8).reshape(n, 40)
    _, first = np.unique(x, axis=0, return_index=True)
    assert len(first) == n, "boards are not distinct"
    return x
