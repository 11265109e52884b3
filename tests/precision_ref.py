"""CPU models of the MFMA towers NET_BF16 / NET_F16 and NET_F32X (TEST INFRASTRUCTURE, not a conftest).

NET_BF16 / NET_F16 (`forward`):

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
`lattice_net` builds nets that pass it.

NET_F32X (`forward_fx`, a third element beside BF16 / F16) follows csrc/azr_tower_fx.hip and net_fx_upload: fp32 stem (no 16-bit
rounding of the planes), per layer the scale 2^e of net_fx_upload, weights and activations as fp16 pairs hi = rne16(x),
lo = rne16(x - hi), acc = sum (ah wh + al wh + ah wl) without al wl, fmaf epilogue, the shortcut added from the fp32 value of the
block input (not from its pair), heads in float64 on hi + lo.  Its certificate (`_certify_terms`) is taken from the products that
occur, per output; `lattice_net_fx` builds nets of two channel families (coarse, al = 0; rich, al != 0, fed by rich weights with
wl != 0 on coarse channels and by ternary weights on rich ones) that pass it while every fragment position of the layer loop meets
both cross terms (`_fx_coverage`); `variant=` are the mistakes a test of that kernel has to see.  It pins the kernel's packing,
term placement, operand timing, skip masks, shortcut operand and layer scale bit for bit up to the fp32 noise of the heads."""
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


def _lattice_heads(rng, out, g):
    """the dense heads of the lattice nets: logits O(1) and a value pre-activation O(0.5) on tower outputs of size g"""
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
    _lattice_heads(rng, out, np.float32(1.25 ** blocks if head_gain is None else head_gain))   # the activations grow by about 1.25 per block
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


# ---------------------------------------------------------------------------------------------------------------------------------
# NET_F32X: the fp16-pair element (csrc/azr_tower_fx.hip, k_tower_fx<2> and net_fx_upload)
# ---------------------------------------------------------------------------------------------------------------------------------
F32X = Elem("f32x", None, None, 2.0 ** -5)   # no 16-bit rounding of its own: operands are pairs; q = the coarse quantum of lattice_net_fx
ELEMS["f32x"] = F32X

FX_VARIANTS = ("drop_wh_al", "drop_wl_ah", "wl_ah_next_tile", "stale_al", "shortcut_pair", "with_al_wl")


def split_pair(x):
    """split_pair of azr_tower_fx.hip (and the weight split of net_fx_upload): hi = rne16(x), lo = rne16(x - (float)hi), the
    subtraction in fp32 (exact); float32 values of both halves.  fp16 subnormals keep their value"""
    x = np.asarray(x, np.float32)
    hi = h2f(f2h(x))
    with np.errstate(invalid="ignore"):
        lo = h2f(f2h(x - hi))
    return hi, lo


def _lowbit_exp(x):
    """exponent of the lowest set bit of every entry of the float64 array x (x = odd * 2^e); +inf for zeros"""
    x = np.asarray(x, np.float64)
    m, e = np.frexp(x)
    mi = np.abs(m * 2.0 ** 53).astype(np.int64)
    lb = np.frexp((mi & -mi).astype(np.float64))[1] - 1
    return np.where(x == 0, np.inf, (lb + e - 53).astype(np.float64))


def _minplus_conv(Ea, Ew):
    """min over the products that occur of (lowbit exponent of a) + (lowbit exponent of w), per output: Ea [n, 7, 6, Cin] and
    Ew [3, 3, Cin, Cout] hold +inf where the operand is zero.  Enumerated through the non-zero weights: per tap a table of the
    k-th input channel of every output channel (channel Cin = a channel of zeros where an output has fewer)"""
    n, cin, cout = Ea.shape[0], Ew.shape[2], Ew.shape[3]
    ap = torch.nn.functional.pad(torch.from_numpy(Ea), (0, 1, 1, 1, 1, 1), value=float("inf"))
    out = torch.full((n, 7, 6, cout), float("inf"), dtype=ap.dtype)
    for ky in range(3):
        for kx in range(3):
            fin = np.isfinite(Ew[ky, kx])
            K = int(fin.sum(0).max())
            if K == 0:
                continue
            order = np.argsort(~fin, axis=0, kind="stable")[:K]              # [K, Cout]: the non-zero input channels first
            ew = np.take_along_axis(Ew[ky, kx], order, 0)                    # inf where an output has fewer than K
            idx = np.where(np.isfinite(ew), order, cin)
            P = ap[:, ky:ky + 7, kx:kx + 6, :][..., torch.from_numpy(idx)] + torch.from_numpy(ew)   # [n, 7, 6, K, Cout]
            out = torch.minimum(out, P.amin(3))
    return out


def _certify_terms(tag, families, acc, stats):
    """the certificate from the products that actually occur.  families = [((a, ...), W), ...]: every term a * w of every family that
    enters one output is a multiple of that output's quantum q = the smallest lowest-set-bit of its terms (a product of two
    dyadic numbers has the product of their lowest bits as its lowest bit), sum |term| < 2^24 q and q >= 2^-149: then every partial
    sum of every order is an exact fp32 number and acc (float64) is THE fp32 sum of that output"""
    emin, bound = None, None
    for acts, W in families:
        acts, W = [np.asarray(a, np.float64) for a in acts], np.asarray(W, np.float64)
        # operands that meet the same weights share one pass: min and sum go through the conv
        e = _minplus_conv(np.minimum.reduce([_lowbit_exp(a) for a in acts]).astype(np.float32), _lowbit_exp(W).astype(np.float32))
        b = conv3x3(torch.from_numpy(np.add.reduce([np.abs(a) for a in acts])), np.abs(W))
        emin = e if emin is None else torch.minimum(emin, e)
        bound = b if bound is None else bound + b
    has = torch.isfinite(emin)
    if not has.any():
        stats.append(dict(layer=tag, ratio=0.0))
        return
    q = torch.exp2(emin[has].to(torch.float64))
    r = bound[has] / (2.0 ** 24 * q)
    worst = int(torch.argmax(r))
    ratio, qmin = float(r[worst]), float(q.min())
    stats.append(dict(layer=tag, ratio=ratio, q=qmin))
    if not (ratio < 1.0 and qmin >= 2.0 ** -149):
        raise NotExact(f"{tag}: an output's sum |term| = {float(bound[has][worst]):.6g} is not below 2^24 x its quantum "
                       f"{float(q[worst]):.3g} (ratio {ratio:.3g}; smallest quantum {qmin:.3g})")
    assert torch.equal(acc, acc.to(torch.float32).to(torch.float64)), tag


_BORDER = np.zeros((7, 6), bool)
_BORDER[[0, 6], :] = True
_BORDER[:, [0, 5]] = True


def _fx_coverage(hi, lo, wh, wl, rich):
    """which fragment positions (tap, 32-channel k-slice, 16-channel column tile) of one conv layer are live on these boards:
    "rich": a weight with wl != 0 meets a non-zero ah; "tern": a weight with wl == 0 meets an activation with al != 0 (on some
    board, in some cell; rich_n / tern_n count these products); cell_*[tap] = (in a border cell, in an interior cell) of the board, by OUTPUT cell; enter / enter_lo =
    the non-zero activations that enter the wl == 0 weights reading a channel of `rich`, and those of them with al != 0"""
    nzh = np.pad(hi != 0, ((0, 0), (1, 1), (1, 1), (0, 0)))
    nzl = np.pad(lo != 0, ((0, 0), (1, 1), (1, 1), (0, 0)))
    nza = np.pad((hi != 0) | (lo != 0), ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = dict(rich_n=np.zeros((9, 8, 16), np.int64), tern_n=np.zeros((9, 8, 16), np.int64), cell_rich=np.zeros((9, 2), bool),
               cell_tern=np.zeros((9, 2), bool), enter=0, enter_lo=0)
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        for kind, sel, src in (("rich", wl[ky, kx] != 0, nzh), ("tern", (wl[ky, kx] == 0) & (wh[ky, kx] != 0), nzl)):
            ci, co = np.nonzero(sel)
            if len(ci) == 0:
                continue
            view = src[:, ky:ky + 7, kx:kx + 6, :]
            cells = view.sum(0)[:, :, ci]                                # [7, 6, weights]: boards on which the product is live
            np.add.at(out[kind + "_n"], (tap, ci // 32, co // 16), cells.sum((0, 1)))
            out["cell_" + kind][tap] |= [cells[_BORDER].any(), cells[~_BORDER].any()]
            if kind == "tern":
                r = ci[rich[ci]]
                out["enter"] += int(nza[:, ky:ky + 7, kx:kx + 6, :].sum((0, 1, 2))[r].sum())
                out["enter_lo"] += int(view.sum((0, 1, 2))[r].sum())
    out["rich"], out["tern"] = out["rich_n"] > 0, out["tern_n"] > 0
    return out


def forward_fx(flat, blocks, in88, rounding=True, certify=False, return_tower=False, variant=None, coverage=False, rich=None):
    """pi [n, 43], v [n] (float64) of NET_F32X on the boards in88 [n, 88], and stats.  It follows k_tower_fx<2> and net_fx_upload:
      * stem: fp32 planes (plane_value, no 16-bit rounding) and fp32 weights on the fp32-input MFMA, the fold indexed by the board row;
      * conv layer L: e as in net_fx_upload (= f16_scale), w' = w * 2^e in fp32, wh = rne16(w'), wl = rne16(w' - wh), 2^-e
        multiplied into the folded BN scale (exact); acc = sum (ah wh + al wh + ah wl) — al wl is not computed;
      * epilogue: y = fmaf(acc, s, shift) (one rounding); on the second conv of a block + the block input, which is the fp32 y of
        the previous block's output (registers), one more rounding; ReLU; hi = rne16(y), lo = rne16(y - hi): the next layer's
        operand is the pair, the next block's shortcut the fp32 y;
      * heads: float64 on hi + lo of the last layer.
    rounding=False: the plain float64 graph.  certify: the exactness certificate from the products that occur (_certify_terms),
    and the fma and the shortcut add exact in float64.  coverage: stats["coverage"][L] = _fx_coverage of conv layer L (`rich` =
    bool [256], the channels whose readers count as rich-reading; default: the rich family of lattice_net_fx).
    variant (none of them is what the kernel does) = dict(kind=..., layer=L, tap=t, ks=k, ct=c), restricted to one layer, tap,
    32-channel k-slice and 16-channel column tile: "drop_wh_al", "drop_wl_ah", "wl_ah_next_tile" (added into column tile c ^ 1
    instead), "stale_al" (al read from k-slice k - 1 of the tap; k >= 1); or dict(kind=...) for the whole net: "shortcut_pair"
    (the shortcut taken from hi + lo), "with_al_wl"."""
    p = _params(flat, blocks)
    stats = dict(layers=[], density=[], vmax=[], exps=[], coverage=[], lo_share=[])
    kind = None if variant is None else variant["kind"]
    assert kind is None or kind in FX_VARIANTS, kind
    if rich is None:
        rich = fx_families()[0]

    def fold(bn, unscale):
        if not rounding:
            g, b, m, v = (np.asarray(bn[i], np.float64) for i in range(4))
            s = g / np.sqrt(v + 1e-3)
            return s, b - m * s
        s, sh = fold_bn32(bn)
        return (s * np.float32(unscale)).astype(np.float32), sh

    def epilogue(tag, acc, s, sh, res=None):
        acc = acc.numpy().astype(np.float64)
        if not rounding:
            return np.maximum(acc * s + sh + (0.0 if res is None else res), 0.0)
        s64, sh64 = np.asarray(s, np.float64), np.asarray(sh, np.float32).astype(np.float64)
        t = acc * s64
        if certify and not two_sum_exact(t, np.broadcast_to(sh64, t.shape)).all():
            raise NotExact(f"{tag}: fmaf(acc, s, shift) is not exact in float64")
        v = (t + sh64).astype(np.float32)
        if res is not None:
            r64, v64 = np.asarray(res, np.float64), v.astype(np.float64)
            if certify and not two_sum_exact(v64, r64).all():
                raise NotExact(f"{tag}: the shortcut add is not exact in float64")
            v = (v64 + r64).astype(np.float32)
        y = np.maximum(v, np.float32(0))
        stats["density"].append(float(np.count_nonzero(y)) / y.size)
        stats["vmax"].append(float(y.max()))
        return y

    def local(a, W, tap, ks, ct, src_ks=None):
        ky, kx = divmod(tap, 3)
        k0 = (ks if src_ks is None else src_ks) * 32
        S = _pad(a)[:, ky:ky + 7, kx:kx + 6, k0:k0 + 32]
        return S @ torch.from_numpy(np.asarray(W[ky, kx, ks * 32:ks * 32 + 32, ct * 16:ct * 16 + 16], np.float64))

    # stem
    x = np.ascontiguousarray(R.planes_from_in88(in88).transpose(0, 2, 3, 1)).astype(np.float64)
    W = np.asarray(p["stem_w"], np.float32).astype(np.float64)
    acc = conv3x3(torch.from_numpy(x), W)
    if certify:
        _certify_terms("stem", [((x,), W)], acc, stats["layers"])
    s, sh = fold(p["stem_bn"], 1.0)
    y = epilogue("stem", acc, s.reshape(1, 7, 1, 1), sh.reshape(1, 7, 1, 1))
    res = y                                                  # the block input: fp32, and (a variant's only) its pair
    res_hi, res_lo = split_pair(y) if rounding else (y, 0.0)
    # tower
    for L in range(2 * blocks):
        name = f"b{L // 2}{'ab'[L & 1]}"
        W32 = np.asarray(p[name + "_w"], np.float32)
        if not rounding:
            acc = conv3x3(torch.from_numpy(y), W32.astype(np.float64))
            s, sh = fold(p[name + "_bn"], 1.0)
            y = epilogue(name, acc, s, sh, res if L & 1 else None)
            if L & 1:
                res = y
            continue
        e = f16_scale(W32)                                   # net_fx_upload computes the same exponent
        stats["exps"].append(e)
        wh, wl = split_pair(W32 * np.float32(2.0 ** e))
        hi, lo = split_pair(y)
        nz = np.count_nonzero(y)
        stats["lo_share"].append(float(np.count_nonzero(lo)) / max(nz, 1))
        ah, al = torch.from_numpy(hi.astype(np.float64)), torch.from_numpy(lo.astype(np.float64))
        acc = conv3x3(ah + al, wh) + conv3x3(ah, wl)         # ah wh + al wh + ah wl
        if certify:
            _certify_terms(name, [((hi, lo), wh), ((hi,), wl)], acc, stats["layers"])
        if coverage:
            stats["coverage"].append(_fx_coverage(hi, lo, wh, wl, rich))
        if kind == "with_al_wl":
            acc = acc + conv3x3(al, wl)
        elif kind is not None and kind != "shortcut_pair" and variant["layer"] == L:
            tap, ks, ct = variant["tap"], variant["ks"], variant["ct"]
            cs = slice(ct * 16, ct * 16 + 16)
            acc = acc.clone()
            if kind == "drop_wh_al":
                acc[..., cs] -= local(al, wh, tap, ks, ct)
            elif kind == "drop_wl_ah":
                acc[..., cs] -= local(ah, wl, tap, ks, ct)
            elif kind == "wl_ah_next_tile":
                d = local(ah, wl, tap, ks, ct)
                acc[..., cs] -= d
                acc[..., (ct ^ 1) * 16:(ct ^ 1) * 16 + 16] += d
            else:
                assert kind == "stale_al" and ks >= 1, variant
                acc[..., cs] += local(al, wh, tap, ks, ct, src_ks=ks - 1) - local(al, wh, tap, ks, ct)
        s, sh = fold(p[name + "_bn"], 2.0 ** -e)
        r = None
        if L & 1:
            r = (res_hi + res_lo) if kind == "shortcut_pair" else res
        y = epilogue(name, acc, s, sh, r)
        if L & 1:
            res = y
            res_hi, res_lo = split_pair(y)
    if rounding:
        hi, lo = split_pair(y)
        h = hi.astype(np.float64) + lo.astype(np.float64)
    else:
        h = y
    pi, v = heads(p, h)
    if return_tower:
        return pi, v, stats, h
    return pi, v, stats


# ---------------------------------------------------------------------------------------------------------------------------------
# exact nets and boards for the pair
# ---------------------------------------------------------------------------------------------------------------------------------
def fx_families():
    """(rich, tiny) bool [256] of lattice_net_fx: the odd channels are rich, the even ones coarse; the last channel of every
    16-channel tile is tiny: a rich channel that no conv weight reads"""
    c = np.arange(F_)
    return c % 2 == 1, c % 16 == 15


def fx_positions(L, ct, count, kind):
    """the (tap, k-slice) fragment positions of column tile ct in conv layer L that lattice_net_fx fills with `count` groups of
    rich weights (kind 0) / of ternary weights reading rich channels (kind 1): they walk through all 72 in 72 / count layers"""
    return [divmod((count * L + i + 9 * ct + 36 * kind) % 72, 8) for i in range(count)]


def lattice_net_fx(blocks, seed, nnz=2, rich_groups=3, beta=(0.125, 0.75), beta_b=(-0.625, -0.125), stem_fine=2.0 ** -8,
                   head_gain=1.5, rich_head=4.0):
    """an AZRW flat vector whose NET_F32X arithmetic is exact on fx_boards (certificate of forward_fx) and exercises all three
    term families.  Every layer's 256 channels are two families (fx_families):
      coarse (even) channels: `nnz` weights of +-1 reading coarse channels, shifts on the quantum F32X.q = 2^-5: al = 0, few bits;
      rich (odd) channels: activations on the quantum 2^-19 with al != 0.  Each is fed by `rich_groups` RICH weights reading
        coarse channels (w * 2^13 = an odd multiple of 1/2 in [2^12, 1.25 * 2^12): 14 significant bits, wl = +-1.5 — the term
        wl ah), by `rich_groups` weights of +-1 reading rich channels (the term wh al), and a shift on the fine quantum.
    No rich weight reads a rich channel, so the al wl term the kernel leaves out is identically zero.  The largest weight of every
    layer is 1 (e = 13).  The non-zeros are placed, not drawn: the 8 rich channels of column tile ct hold their weights of layer L
    at the same fragment positions fx_positions(L, ct, ...), each on an input channel of its own inside the k-slice.
    Tiny channels (the last of every tile): rich-fed, BN scale 2^-16 and shifts around 2^-16 on the quantum 2^-39, read by no conv
    weight and carried by the shortcut: their fp32 value has bits below 2^-24 that the pair drops — where the shortcut operand
    would show if it were taken from hi + lo; their head weights are 2^16 times the others'.
    Stem: coarse channels read the three army planes (quantum 2^-5), rich ones also two float planes, the second at `stem_fine`;
    the stem's BN is per board row, so its shifts are coarse, and none is positive: -(0 .. 6) / 16.  Heads as lattice_net's, the rich channels' 1x1
    weights `rich_head` times the coarse ones'."""
    rng = np.random.default_rng(seed)
    qa = F32X.q
    rich, tiny = fx_families()
    coarse_i, rich_i, read_i = np.flatnonzero(~rich), np.flatnonzero(rich), np.flatnonzero(rich & ~tiny)
    out = {}
    W = np.zeros((3, 3, 13, F_), np.float32)
    for co in range(F_):
        taps = rng.choice(9, 4, replace=False)
        for i, tp in enumerate(taps[:2 if rich[co] else 4]):
            W[tp // 3, tp % 3, rng.integers(0, 3), co] = rng.choice([-1.0, 1.0])
        if rich[co] and not tiny[co]:
            f1, f2 = rng.choice(10, 2, replace=False) + 3
            W[taps[2] // 3, taps[2] % 3, f1, co] = rng.choice([-1.0, 1.0])
            if stem_fine:
                W[taps[3] // 3, taps[3] % 3, f2, co] = rng.choice([-1.0, 1.0]) * stem_fine
        if tiny[co]:
            W[:, :, :, co] = 0
    out["stem_w"] = W
    stem_b = -rng.permutation(np.arange(7)).astype(np.float32) * np.float32(0.0625)   # none positive: the tiny channels start at 0
    out["stem_bn"] = np.stack([np.ones(7, np.float32), stem_b, np.zeros(7, np.float32), np.full(7, VAR_ONE)])
    for L in range(2 * blocks):
        name = f"b{L // 2}{'ab'[L & 1]}"
        lo, hi = beta_b if L & 1 else beta
        W = np.zeros((9, F_, F_), np.float32)
        for co in coarse_i:
            idx = rng.choice(9 * len(coarse_i), nnz, replace=False)
            sg = rng.permutation(np.arange(nnz) % 2 * 2 - 1) if L & 1 else -np.ones(nnz)
            W[idx // len(coarse_i), coarse_i[idx % len(coarse_i)], co] = sg
        for ct in range(16):
            for kind, pool_i in ((0, coarse_i), (1, read_i)):
                for tap, ks in fx_positions(L, ct, rich_groups, kind):
                    src = pool_i[(pool_i >= ks * 32) & (pool_i < ks * 32 + 32)]
                    ci = rng.permutation(src)[:8]
                    sg = rng.permutation(np.arange(8) % 2 * 2 - 1) if L & 1 else -np.ones(8)
                    # w * 2^13 = 4 k + 1.5 or 4 k + 2.5 in [2^12, 1.25 * 2^12): wh = 4 k or 4 k + 4 and |wl| = 1.5, the largest share of
                    # a weight that a low part can hold short of a tie
                    mag = (4 * rng.integers(1024, 1280, 8) + rng.choice([1.5, 2.5], 8)) * 2.0 ** -13 if kind == 0 else np.ones(8)
                    W[tap, ci, rich_i[rich_i // 16 == ct]] = sg * mag
        out[name + "_w"] = W.reshape(3, 3, F_, F_)
        gamma = np.where(tiny, np.float32(2.0 ** -16), np.float32(1.0)).astype(np.float32)
        shift = _multiples(rng, lo, hi, qa, F_)
        shift[rich] = _multiples(rng, lo, hi, 2.0 ** -19, int(rich.sum()))
        shift[tiny] = (rng.integers(-2 ** 22, 2 ** 23, int(tiny.sum())) * 2.0 ** -39).astype(np.float32)
        out[name + "_bn"] = np.stack([gamma, shift, np.zeros(F_, np.float32), np.full(F_, VAR_ONE)])
    _lattice_heads(rng, out, np.float32(head_gain))
    for k in ("pi_w", "v_w"):
        out[k][rich] *= np.float32(rich_head)
        out[k][tiny] *= np.float32(2.0 ** 16)
    return to_flat(blocks, out)


def fx_boards(n, seed, exact_planes=True):
    """lattice_boards for the pair: float planes on the quantum 2^-11 in [0, 1] — or (exact_planes=False) lattice_boards' planes
    that fp16 cannot represent (ties between two fp16 neighbours included), brought to the quantum 2^-16: the stem keeps them in
    fp32, and sums of them stay exact in fp32"""
    x = lattice_boards(n, seed, F16, exact_planes)
    if not exact_planes:
        f = x[:, 48:88].copy().view(np.float32).reshape(n, 10)
        f = (np.round(f.astype(np.float64) * 2.0 ** 16) * 2.0 ** -16).astype(np.float32)
        x[:, 48:88] = f.view(np.uint8).reshape(n, 40)
        assert len(np.unique(x, axis=0)) == n
    return x


def fx_edge_net(kind, seed):
    """two-block NET_F32X nets at the edges of net_fx_upload's layer scale, exact like lattice_net_fx:
      "scale_clamps": the first conv's weights are 2^-12 times lattice_net_fx's (largest 2^-12: e = 25 -> clamped to 24) with the BN
                      scales 2^12 times, the second's 2^15 times (e = -2) with 2^-15, the third conv all zeros (e = 0)
      "subnormal_wl": in the last conv the rich channels of column tile 5 hold weights 2^-17 times the usual size — the rich ones
                      (2^-4 + j 2^-18) 2^-13, j = 1 .. 3: after the layer scale wh = 2^-4 and wl = j 2^-18, an fp16 subnormal that the
                      matrix core takes at full value — with the BN scale 2^17 times"""
    blocks = 2
    p = from_flat(blocks, lattice_net_fx(blocks, seed))
    if kind == "scale_clamps":
        p["b0a_w"] *= np.float32(2.0 ** -12)
        p["b0a_bn"][0] *= np.float32(2.0 ** 12)
        p["b0b_w"] *= np.float32(2.0 ** 15)
        p["b0b_bn"][0] *= np.float32(2.0 ** -15)
        p["b1a_w"][:] = 0
        return to_flat(blocks, p)
    assert kind == "subnormal_wl", kind
    rng = np.random.default_rng(seed + 13)
    rich, tiny = fx_families()
    cols = np.flatnonzero(rich & ~tiny & (np.arange(F_) // 16 == 5))
    W = p["b1b_w"]
    sub = W[..., cols]
    _, wl = split_pair(sub * np.float32(2.0 ** 13))
    small = np.where(wl != 0, np.sign(sub) * (2.0 ** -4 + rng.integers(1, 4, sub.shape) * 2.0 ** -18) * 2.0 ** -13, sub * 2.0 ** -17)
    W[..., cols] = small.astype(np.float32)
    p["b1b_bn"][0][cols] *= np.float32(2.0 ** 17)
    return to_flat(blocks, p)


_fx_pools = {}


def fx_pool(blocks, boards=256):
    """the lattice net of depth `blocks`, the pool of 256 lattice boards of the GPU test, and the model's pi, v and stats for them
    (certified, with the coverage tables), computed once per process"""
    if (blocks, boards) not in _fx_pools:
        flat = lattice_net_fx(blocks, 5)
        x = fx_boards(boards, 9)
        pi, v, st = forward_fx(flat, blocks, x, certify=True, coverage=True)
        _fx_pools[blocks, boards] = (flat, x, pi, v, st)
    return _fx_pools[blocks, boards]
