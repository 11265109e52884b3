// azr_train_conv.hpp — the tower convs of the optimiser step in split precision: split / pack helpers, the batch-norm arithmetic
// they share with the normalise kernels, t_conv_rs and t_conv_q
// (A private header of azr_train.hip, the one translation unit that includes it: everything here has internal linkage.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "azr_bf16_common.hpp"   // the vector register types
#include "azr_rowclass.hpp"
#include "azr_train_common.hpp"

namespace {

// =====================================================================================================================
// The same GEMM in split bf16 on v_mfma_f32_16x16x32_bf16 (16x the fp32 MFMA rate).  An fp32 value is the exact sum of
// three bf16 parts x = h + m + l (8 + 8 + 8 mantissa bits); t_split writes the parts of an operand once, and
//   NP = 3 (forward):  C += Al*Bh + Ah*Bl + Am*Bm + Am*Bh + Ah*Bm + Ah*Bh   — every product term above 2^-24 relative:
//                      fp32-exact products, so the ReLU masks and batch statistics match an fp32 forward;
//   NP = 2 (backward): C += Am*Bh + Ah*Bm + Ah*Bh                           — 16 bits per factor, 1e-5 relative;
// fp32 accumulation in both.  Tile BM x 128, k-tile 32, 4 waves as 2 x 2, LDS rows [m|n][32 + 8 pad] bf16 per part
// (80-byte stride: an MFMA fragment's ds_read_b128 is conflict-free).  Operand views as in gt_load (MODE 0..3); a
// mn-contiguous operand is transposed in registers (8 dword loads down k, v_perm, two 16-byte LDS writes).
// =====================================================================================================================
constexpr int K3 = 32, KP3 = 40;
struct Parts { const uint16_t* p[3]; };

__device__ __forceinline__ uint32_t bf_rne_bits(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
// two floats -> two bf16 (round to nearest even) packed low | high: ONE v_cvt_pk_bf16_f32 where bf_rne_bits spends three integer
// operations per value and two more to pack — the same bits for every finite input (the staging paths of the fused convs run this for
// every element of every layer: profiles/r04_train_step.txt)
__device__ __forceinline__ uint32_t bf_rne_pk(float a, float b)
{
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{a, b}, bf16x2));
}
// hi and mid bf16 parts of a pair of floats (hi = rne(v), mid = rne(v - hi)), packed
__device__ __forceinline__ void bf_split2(float a, float b, uint32_t& hi, uint32_t& mid)
{
    hi = bf_rne_pk(a, b);
    mid = bf_rne_pk(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u));
}
__device__ __forceinline__ void split_store4(const float (&v)[4], size_t i4, uint16_t* p0, uint16_t* p1, uint16_t* p2)
{
    if (!p2) {   // the two leading parts only (every caller on the step's hot path)
        uint32_t h01, m01, h23, m23;
        bf_split2(v[0], v[1], h01, m01);
        bf_split2(v[2], v[3], h23, m23);
        reinterpret_cast<uint2*>(p0)[i4] = make_uint2(h01, h23);
        reinterpret_cast<uint2*>(p1)[i4] = make_uint2(m01, m23);
        return;
    }
    uint32_t h[4], m[4], l[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        h[j] = bf_rne_bits(v[j]);
        const float r1 = v[j] - __uint_as_float(h[j] << 16);
        m[j] = bf_rne_bits(r1);
        l[j] = bf_rne_bits(r1 - __uint_as_float(m[j] << 16));
    }
    reinterpret_cast<uint2*>(p0)[i4] = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
    reinterpret_cast<uint2*>(p1)[i4] = make_uint2(m[0] | (m[1] << 16), m[2] | (m[3] << 16));
    reinterpret_cast<uint2*>(p2)[i4] = make_uint2(l[0] | (l[1] << 16), l[2] | (l[3] << 16));
}

// the fp16 pair of 4 consecutive values: hi = rne16(v), lo = rne16(v - hi) (unscaled: the matrix core takes fp16 subnormals),
// 22 significand bits — the operand format of the 3-pass forward conv (t_conv_rs<1, 2, 0, true>)
__device__ __forceinline__ void f16_pair4(const float (&v)[4], uint2& hi, uint2& lo)
{   // two values per conversion (v_cvt_pk_f16_f32, RNE: the bits of the scalar conversions)
    const f16x2 h01 = __builtin_convertvector(f32x2{v[0], v[1]}, f16x2), h23 = __builtin_convertvector(f32x2{v[2], v[3]}, f16x2);
    const f16x2 l01 = __builtin_convertvector(f32x2{v[0] - (float)h01[0], v[1] - (float)h01[1]}, f16x2);
    const f16x2 l23 = __builtin_convertvector(f32x2{v[2] - (float)h23[0], v[3] - (float)h23[1]}, f16x2);
    hi = make_uint2(__builtin_bit_cast(uint32_t, h01), __builtin_bit_cast(uint32_t, h23));
    lo = make_uint2(__builtin_bit_cast(uint32_t, l01), __builtin_bit_cast(uint32_t, l23));
}
__device__ __forceinline__ void split_store4_f16(const float (&v)[4], size_t i4, uint16_t* q0, uint16_t* q1)
{
    uint2 hi, lo;
    f16_pair4(v, hi, lo);
    reinterpret_cast<uint2*>(q0)[i4] = hi;
    reinterpret_cast<uint2*>(q1)[i4] = lo;
}

// The batch-norm arithmetic of the step, each formula stated once: the normalise kernels (t_bn_apply, t_bn_bwd_apply), the statistics
// kernels and the fused convs (staging paths and epilogues) all call these, and the library is built without FMA contraction, so the
// source order here IS the rounding order of every one of them (test_fused_normalise_kernels_change_no_bit).
__device__ __forceinline__ float bn_xhat(float y, float mean, float istd) { return (y - mean) * istd; }
// A = relu(gamma * xhat + beta + s)
__device__ __forceinline__ float bn_fwd(float y, float s, float gamma, float beta, float mean, float istd)
{
    const float v = gamma * bn_xhat(y, mean, istd) + beta + s;
    return v > 0.0f ? v : 0.0f;
}
// dY = gamma * istd * (dz - sum(dz)/n - xhat * sum(dz xhat)/n), dz = dOut where the post-activation is positive
__device__ __forceinline__ float bn_bwd(float dOut, float apost, float y, float gamma, float mean, float istd, float s_n, float sx_n, float& dz)
{
    dz = apost > 0.0f ? dOut : 0.0f;
    return gamma * istd * (dz - s_n - bn_xhat(y, mean, istd) * sx_n);
}
// one element's share of the statistics, in double: sum and sum of squares (forward), sum dz and sum dz * xhat (backward; the caller
// masks dz, so that a kernel which reads dOut from memory keeps its load behind the test of the post-activation)
__device__ __forceinline__ void bn_stat_fwd(float y, double& s, double& ss)
{
    const double v = (double)y;
    s += v;
    ss += v * v;
}
__device__ __forceinline__ void bn_stat_bwd(float dz, float y, float mean, float istd, double& s, double& sx)
{
    s += (double)dz;
    sx += (double)dz * (double)bn_xhat(y, mean, istd);
}
// a conv epilogue's partials: the 16 lanes c = 0..15 of a channel group hold different cells — butterfly over c, lane c = 0 writes
// part[row][2][256] (the sums of a lane's own cells came first: the order is part of the result)
template <typename Row>
__device__ __forceinline__ void part_butterfly_store(double (&s)[4], double (&sx)[4], int c, double* part, Row row, int ch0)
{
#pragma unroll
    for (int e = 0; e < 4; e++) {
#pragma unroll
        for (int sft = 1; sft < 16; sft <<= 1) {
            s[e] += __shfl_xor(s[e], sft);
            sx[e] += __shfl_xor(sx[e], sft);
        }
        if (c == 0) {
            part[((size_t)row * 2 + 0) * NF + ch0 + e] = s[e];
            part[((size_t)row * 2 + 1) * NF + ch0 + e] = sx[e];
        }
    }
}

// =====================================================================================================================
// Conv GEMMs whose B operand is the layer's kernel (forward, backward-data): N = 256, K = 2304.  The measured limit of
// t_gemm_sb on these shapes is LDS traffic, two thirds of it the weight tile.  Here the weights never touch LDS: t_pack_w
// writes their bf16 parts once per step in MFMA-fragment order ([k-tile][n-tile][lane][8]) and every wave loads the
// fragments of ITS 32 columns straight from global memory (1 KB coalesced per fragment, register double buffer).  Block =
// 64 rows x 128 columns, 4 waves side by side (64 x 32 each); only the activation tile goes through LDS.
//   VIEW 0: forward        B[k = tap*256+ci][n = co] = W[tap][ci][co]
//   VIEW 1: backward-data  B[k = tap*256+co][n = ci] = W[tap][ci][co]
// =====================================================================================================================
constexpr size_t WPACK = (size_t)KC * NF;  // elements per layer, part and view

// wscale > 0: fp16 PAIRS of wscale * W instead of bf16 parts (p0 = hi, p1 = lo; the forward conv on the fp16 MFMA)
template <int NP>
__global__ __launch_bounds__(256) void t_pack_w(const float* __restrict__ flat, int view, uint16_t* __restrict__ p0, uint16_t* __restrict__ p1,
                                                uint16_t* __restrict__ p2, float wscale = 0.0f, int* __restrict__ range_flag = nullptr)
{
    // one thread = one lane's 8 values of one fragment: index = ((kt * 16 + nt) * 64 + lane)
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= WPACK / 8) return;
    const int l = blockIdx.y;
    const float* W = flat + OFF_BLOCK0 + (size_t)l * LAYER;
    const int lane = (int)(i & 63), nt = (int)((i >> 6) & 15), kt = (int)(i >> 10);
    const int n = nt * 16 + (lane & 15), k0 = kt * 32 + (lane >> 4) * 8, tap = k0 >> 8, c0 = k0 & 255;
    uint32_t h[8], m[8], lo[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const float v = view == 0 ? W[((size_t)tap * NF + (c0 + j)) * NF + n]    // ci = c0 + j, co = n
                                  : W[((size_t)tap * NF + n) * NF + (c0 + j)];   // ci = n, co = c0 + j
        if (wscale > 0.0f) {
            const float vs = v * wscale;
            // a weight that leaves the fp16 range (|w| >= 64 at the 2^10 scale) or is not a number would turn into inf / NaN here and
            // poison the step silently: raise the step's range flag instead (read by the caller behind the epoch)
            if (!(fabsf(vs) < 65504.0f) && range_flag) atomicOr(range_flag, 1);
            const _Float16 hh = (_Float16)vs, ll = (_Float16)(vs - (float)hh);
            h[j] = __builtin_bit_cast(uint16_t, hh);
            m[j] = __builtin_bit_cast(uint16_t, ll);
            lo[j] = 0u;
            continue;
        }
        h[j] = bf_rne_bits(v);
        const float r1 = v - __uint_as_float(h[j] << 16);
        m[j] = bf_rne_bits(r1);
        lo[j] = bf_rne_bits(r1 - __uint_as_float(m[j] << 16));
    }
    const size_t o = (size_t)l * (WPACK / 8) + i;
    reinterpret_cast<uint4*>(p0)[o] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
    reinterpret_cast<uint4*>(p1)[o] = make_uint4(m[0] | (m[1] << 16), m[2] | (m[3] << 16), m[4] | (m[5] << 16), m[6] | (m[7] << 16));
    if (NP == 3) reinterpret_cast<uint4*>(p2)[o] = make_uint4(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16), lo[4] | (lo[5] << 16), lo[6] | (lo[7] << 16));
}

// ---------------------------------------------------------------------------------------------------------------------
// t_conv_rs: the same two conv GEMMs (forward, backward-data) with what the inference tower (azr_tower_sb.hip) taught:
//   * a block owns 2 boards = 84 rows in BORDER-CLASS order (azr_rowclass.hpp, 6 MFMA row tiles): the 9 of 54 (tile, tap)
//     pairs that lie wholly outside the board are not issued (17 % of the MFMAs and fragment reads);
//   * 4 waves x 64 output channels (four 16-wide tiles): an activation fragment read from LDS feeds 4 MFMAs per pass,
//     and MFMA(weights, activations) leaves 4 consecutive channels of one cell in a lane: 16-byte stores;
//   * K order = channel chunk outermost (8 chunks of 32 input channels), tap innermost: only the current 32-channel slice
//     of the 84 rows has to be in LDS (two buffers; the next slice is fetched during the 9 k-steps of the current one):
//     ONE barrier per 9 k-steps; the 9 taps are unrolled with compile-time skip masks, the chunk loop is rolled;
//   * weights straight from global memory in MFMA-fragment order (t_pack_w) through a ring of 3 k-steps, refill loads
//     and fragment re-reads dealt out one per pass instead of as bursts.
// AMODE 1: C[row] = sum_tap A[row + tap] W[tap]; AMODE 2 (backward-data): negated taps, i.e. loop index t reads the
// geometric tap 8 - t, with the transposed kernel view.  `boards` = rows / 42 (the last block may hold one board).
// ---------------------------------------------------------------------------------------------------------------------
template <int NP> struct RsPass;
template <> struct RsPass<3> { static constexpr int N = 6; static constexpr int QA[6] = {2, 0, 1, 1, 0, 0}, QB[6] = {0, 2, 1, 0, 1, 0}; };
template <> struct RsPass<2> { static constexpr int N = 3; static constexpr int QA[3] = {1, 0, 0}, QB[3] = {0, 1, 0}; };

// geometry of t_conv_rs (below)
struct Rs {
    static constexpr int NB = 2, ROWS = 84, MT = 6, ZR = 96, NT = 4, RING = 3;
    static constexpr int CHB = 80;                       // bytes per row of a 32-channel slice (64 + 16 pad)
    static constexpr int PB = (ZR + 1) * CHB;            // one part of one slice, incl. the shared zero row
    static constexpr uint32_t KB = 16 * 64 * 16;         // bytes of one k-step of packed weights (16 column tiles x 64 lanes x 16 B)
};

// one MFMA of the conv kernels: packed weight fragment x activation fragment, fp16 pairs (F16) or bf16 parts
template <bool F16>
__device__ __forceinline__ f32x4 mfma_part(const u32x4& b, const s16x8& a, const f32x4& acc)
{
    if constexpr (F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, b), __builtin_bit_cast(f16x8, a), acc, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, b), __builtin_bit_cast(bf16x8, a), acc, 0, 0, 0);
}

// one k-step (one tap of one 32-channel slice) of t_conv_rs; everything that depends on the tap is a compile-time constant
template <int AMODE, int NP, int TAP, bool F16 = false>
__device__ __forceinline__ void rs_tap(const uint8_t* bufc, int kc, const __amdgpu_buffer_rsrc_t (&wsrc)[NP], uint32_t loff,
                                       const uint32_t (&arow)[9][Rs::MT], u32x4 (&bq)[Rs::RING][NP][Rs::NT], f32x4 (&acc)[Rs::MT][Rs::NT],
                                       s16x8 (&a)[Rs::MT][NP])
{
    constexpr int NB = Rs::NB, MT = Rs::MT, NT = Rs::NT, RING = Rs::RING, PB = Rs::PB, NPASS = RsPass<NP>::N;
    constexpr uint32_t sk = skip_mask<NB>(AMODE == 2 ? 8 - TAP : TAP);
    constexpr uint32_t skn = TAP < 8 ? skip_mask<NB>(AMODE == 2 ? 7 - TAP : TAP + 1) : 0xffffffffu;
    constexpr int active = MT - __builtin_popcount(sk & ((1u << MT) - 1u));
    constexpr int cur = TAP % RING, ref = (TAP + RING - 1) % RING;
    // the k-step RING - 1 ahead in consumption order (chunk-major): tap + 2 of this chunk or tap - 7 of the next
    constexpr int tap2 = (TAP + RING - 1) % 9;
    const uint32_t koff = (uint32_t)(tap2 * 8 + kc + (TAP + RING - 1 >= 9 ? 1 : 0)) * Rs::KB;   // (past the layer: out of range -> 0)
    constexpr int slots = active * NPASS;
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        if (!((sk >> mt) & 1u)) {
            const int j = __builtin_popcount(~sk & ((1u << mt) - 1u));
#pragma unroll
            for (int p = 0; p < NPASS; p++) {
                const int qa = RsPass<NP>::QA[p], qb = RsPass<NP>::QB[p];
#pragma unroll
                for (int nt = 0; nt < NT; nt++) acc[mt][nt] = mfma_part<F16>(bq[cur][qb][nt], a[mt][qa], acc[mt][nt]);
                // one refill load of the ring slot the previous k-step freed, dealt out over the k-step
                const int s2 = j * NPASS + p;
#pragma unroll
                for (int i = 0; i < NP * NT; i++)
                    if (s2 == ((i + 1) * slots) / (NP * NT) - 1)
                        bq[ref][i / NT][i % NT] = __builtin_amdgcn_raw_buffer_load_b128(wsrc[i / NT], loff + (i % NT) * 1024, (int)koff, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (!((skn >> mt) & 1u)) {   // this tile's fragments for the next tap
#pragma unroll
                for (int q = 0; q < NP; q++) a[mt][q] = *reinterpret_cast<const s16x8*>(bufc + q * PB + arow[TAP < 8 ? TAP + 1 : 0][mt]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int mt = 0; mt < MT; mt++)   // tiles idle in this tap that run in the next
        if (((sk >> mt) & 1u) && !((skn >> mt) & 1u)) {
#pragma unroll
            for (int q = 0; q < NP; q++) a[mt][q] = *reinterpret_cast<const s16x8*>(bufc + q * PB + arow[TAP < 8 ? TAP + 1 : 0][mt]);
        }
}

// What the backward-data conv of layer l can do for layer l - 1 on its way out (FUSE = 1): its output rows are layer l - 1's
// dOut, still in registers — the shortcut gradient joins them here (first conv of a block: + DS, the job of t_add), and
// stage 1 of layer l - 1's batch-norm backward (t_bn_bwd_stats: per channel sum of dz and of dz * xhat, dz = dOut where the
// post-activation is positive) is taken per block of 2 boards, in double, in a fixed order: cells of a lane, then the 16
// lanes of a channel group.  part[blockIdx][2][256] is what t_bn_bwd_finalize / t_parts_sum read (R = number of blocks).
struct BwdFuse {
    const float* DS;      // shortcut gradient to add to the output rows, or null
    const float* Apost;   // layer l - 1: post-activation, pre-BN conv output, batch mean / 1 / std per channel
    const float* Y;
    const float* mean;
    const float* istd;
    double* part;
};

// What the conv can do on the way IN (PRO): its A operand is an elementwise function of tensors that are complete once the
// batch statistics are — so instead of a kernel that writes the operand parts and this one reading them back, the staging path
// computes them (each block stages every element of its 2 boards exactly once) and writes what later kernels still need:
//   PRO = 1 (forward conv of layer l): A_{l-1} = relu(gamma (Y_{l-1} - mean) istd + beta (+ S)) — t_bn_apply's arithmetic — goes
//            to LDS as fp16 pair; side outputs: A_{l-1} in fp32 (backward masks, shortcut, heads) and its bf16 hi / mid parts (the
//            weight-gradient GEMM's operand);
//   PRO = 2 (backward-data conv of layer l): dY_l = gamma istd (dz - sum(dz)/n - xhat sum(dz xhat)/n), dz = dOut where the
//            post-activation is positive — t_bn_bwd_apply's arithmetic — goes to LDS as bf16 hi / mid; side outputs: those two parts
//            (the weight-gradient GEMM, launched AFTER this kernel) and dz itself where the layer closes a block (the shortcut
//            gradient DS).
struct ProFuse {
    const float* X;       // PRO 1: Y_{l-1}   | PRO 2: dOut_l
    const float* S;       // PRO 1: shortcut input or null | PRO 2: Apost_l
    const float* Y;       // PRO 2: Y_l
    const float* mean;    // per channel [256]
    const float* istd;
    const float* bn;      // gamma | beta
    const float* sums;    // PRO 2: [2][256] sum(dz), sum(dz xhat)
    float inv_count;      // PRO 2
    float* O;             // PRO 1: A_{l-1} (fp32) | PRO 2: dz (DS) or null
    uint16_t* p0;         // bf16 hi / mid parts of the computed operand
    uint16_t* p1;
};
// the per-channel parameters of PRO in LDS: gamma | beta (PRO 1) or sum(dz)/n (PRO 2) | mean | 1/std | (PRO 2) sum(dz xhat)/n
template <int PRO>
__device__ __forceinline__ void ptab_fill(const ProFuse& Pf, float* ptab, int tid)
{
    for (int i = tid; i < NF; i += 256) {
        ptab[i] = Pf.bn[i];
        ptab[2 * NF + i] = Pf.mean[i];
        ptab[3 * NF + i] = Pf.istd[i];
        if constexpr (PRO == 1) ptab[NF + i] = Pf.bn[NF + i];
        else { ptab[NF + i] = Pf.sums[i] * Pf.inv_count; ptab[4 * NF + i] = Pf.sums[NF + i] * Pf.inv_count; }
    }
}
// The operand of PRO from the fp32 sources of the 4 channels ch .. ch + 3 of one cell (xa = X, xb = S, xc = Y: see ProFuse): hi / lo are
// the two words per part that go to LDS; `go` is the cell's element offset in the tensors, and the side outputs are written where
// `side` holds (each element by exactly one block).
template <int PRO>
__device__ __forceinline__ void pro_operand(const ProFuse& Pf, const float* ptab, int ch, size_t go, bool side, const float (&xa)[4],
                                            const float (&xb)[4], const float (&xc)[4], uint2& hi, uint2& lo)
{
    const float4 ga = *reinterpret_cast<const float4*>(ptab + ch), p1 = *reinterpret_cast<const float4*>(ptab + NF + ch),
                 mu = *reinterpret_cast<const float4*>(ptab + 2 * NF + ch), is = *reinterpret_cast<const float4*>(ptab + 3 * NF + ch);
    const float g4[4] = {ga.x, ga.y, ga.z, ga.w}, q4[4] = {p1.x, p1.y, p1.z, p1.w}, m4[4] = {mu.x, mu.y, mu.z, mu.w}, i4[4] = {is.x, is.y, is.z, is.w};
    float o[4];
    if constexpr (PRO == 1) {   // t_bn_apply<false>, as fp16 pair
#pragma unroll
        for (int j = 0; j < 4; j++) o[j] = bn_fwd(xa[j], xb[j], g4[j], q4[j], m4[j], i4[j]);
        f16_pair4(o, hi, lo);
        if (side) {
            *reinterpret_cast<float4*>(Pf.O + go) = make_float4(o[0], o[1], o[2], o[3]);
            split_store4(o, go / 4, Pf.p0, Pf.p1, nullptr);
        }
    } else {                    // t_bn_bwd_apply<false>, as bf16 hi / mid
        const float4 s1 = *reinterpret_cast<const float4*>(ptab + 4 * NF + ch);
        const float t4[4] = {s1.x, s1.y, s1.z, s1.w};
        float z[4];
#pragma unroll
        for (int j = 0; j < 4; j++) o[j] = bn_bwd(xa[j], xb[j], xc[j], g4[j], m4[j], i4[j], q4[j], t4[j], z[j]);
        bf_split2(o[0], o[1], hi.x, lo.x);
        bf_split2(o[2], o[3], hi.y, lo.y);
        if (side) {
            reinterpret_cast<uint2*>(Pf.p0)[go / 4] = hi;
            reinterpret_cast<uint2*>(Pf.p1)[go / 4] = lo;
            if (Pf.O) *reinterpret_cast<float4*>(Pf.O + go) = make_float4(z[0], z[1], z[2], z[3]);
        }
    }
}

// F16: the operands are fp16 pairs (NP = 2: hi, lo) on v_mfma_f32_16x16x32_f16 and the sums are multiplied by `oscale` on the way
// out (the packed kernel carries a power-of-two scale) — the forward conv in 3 passes instead of the 6 of three bf16 parts.
template <int AMODE, int NP, int FUSE = 0, bool F16 = false, int PRO = 0>
__global__ __launch_bounds__(256, 1) void t_conv_rs(Parts A, Parts Bp, float* __restrict__ C, int boards, BwdFuse F = BwdFuse{}, float oscale = 1.0f,
                                                    ProFuse Pf = ProFuse{})
{
    constexpr int NB = Rs::NB, ROWS = Rs::ROWS, MT = Rs::MT, ZR = Rs::ZR, NT = Rs::NT, RING = Rs::RING, CHB = Rs::CHB, PB = Rs::PB;
    constexpr int UN = (NP * ROWS * 4 + 255) / 256;   // 16-byte units of a slice per thread
    constexpr uint32_t KB = Rs::KB;
    __shared__ __attribute__((aligned(16))) uint8_t img[2 * NP * PB];
    __shared__ uint8_t rowof[ROWS];
    __shared__ uint8_t taprow[9 * ZR];
    __shared__ uint16_t rowcell[ZR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    const int b0 = blockIdx.x * NB, m0 = b0 * NPOS;
    const int nbv = boards - b0 < NB ? boards - b0 : NB;

    // ---- weight ring: the first two k-steps (chunk 0, taps 0 and 1) fly while the tables are built
    __amdgpu_buffer_rsrc_t wsrc[NP];
#pragma unroll
    for (int q = 0; q < NP; q++) wsrc[q] = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(Bp.p[q]), (short)0, (int)(WPACK * 2), 0x00020000);
    const uint32_t loff = (uint32_t)((wave * NT) * 64 + lane) * 16u;
    u32x4 bq[RING][NP][NT];
#pragma unroll
    for (int s2 = 0; s2 < RING - 1; s2++)
#pragma unroll
        for (int q = 0; q < NP; q++)
#pragma unroll
            for (int nt = 0; nt < NT; nt++) bq[s2][q][nt] = __builtin_amdgcn_raw_buffer_load_b128(wsrc[q], loff + nt * 1024, (int)((s2 * 8) * KB), 0);

    // ---- tables (the rules of build_row_tables, azr_rowclass.hpp, in this kernel's own loops: through the helper its register numbers
    // change up to the end of its text — profiles/tower_common_isa.txt)
    for (int i = tid; i < ZR; i += 256) rowcell[i] = 0xffffu;
    for (int i = tid; i < 2 * NP * (CHB / 4); i += 256) {   // the zero rows of both buffers
        const int bp = i / (CHB / 4), w4 = i % (CHB / 4);
        reinterpret_cast<uint32_t*>(img + bp * PB + ZR * CHB)[w4] = 0u;
    }
    __syncthreads();
    for (int i = tid; i < ROWS; i += 256) {
        const int b = i / NPOS, pos = i - b * NPOS, r = row_of<NB>(b, pos);
        rowof[i] = (uint8_t)r;
        rowcell[r] = (uint16_t)cell_code(b, pos);
    }
    __syncthreads();
    for (int i = tid; i < 9 * ZR; i += 256) {
        const int t = i / ZR, r = i - t * ZR;
        taprow[i] = (uint8_t)tap_source_row<9>(t, rowcell[r], ZR, rowof);
    }
    // this thread's units of a slice.  PRO = 0: (part, cell, 16-byte segment of 8 halfs) -> global element offset (chunk 0) and LDS
    // byte offset.  PRO != 0: (cell, 4 channels): the fp32 sources are fetched, the operand is computed when the slice is stashed.
    constexpr int UNR = PRO ? (ROWS * 8 + 255) / 256 : UN;
    size_t goff[UNR];
    uint32_t loffs[UNR];
    bool uok[UNR];
    __shared__ __attribute__((aligned(16))) float ptab[PRO ? 5 * NF : 4];   // PRO: per-channel parameters of the elementwise function
    if constexpr (PRO == 0) {
#pragma unroll
        for (int i = 0; i < UN; i++) {
            const int u = tid + 256 * i, q = u / (ROWS * 4), rem = u - q * (ROWS * 4), cell = rem >> 2, seg = rem & 3;
            uok[i] = u < NP * ROWS * 4 && cell < nbv * NPOS;
            goff[i] = (size_t)(m0 + cell) * NF + seg * 8;
            loffs[i] = (uint32_t)((u < NP * ROWS * 4 ? q : 0) * PB + (u < NP * ROWS * 4 ? rowof[cell] : 0) * CHB + seg * 16);
        }
    } else {
        static_assert(NP == 2, "the computed operand has two parts");
#pragma unroll
        for (int i = 0; i < UNR; i++) {
            const int u = tid + 256 * i, cell = u >> 3, seg = u & 7;
            uok[i] = u < ROWS * 8 && cell < nbv * NPOS;
            goff[i] = (size_t)(m0 + cell) * NF + seg * 4;
            loffs[i] = (uint32_t)((u < ROWS * 8 ? rowof[cell] : 0) * CHB + seg * 8);
        }
        ptab_fill<PRO>(Pf, ptab, tid);
        __syncthreads();
    }
    struct Raw { uint4 a, b, c; };   // PRO = 0: a = 16 bytes of a part.  PRO 1: a = Y, b = S.  PRO 2: a = dOut, b = Apost, c = Y
    auto fetch = [&](int kc, Raw (&r)[UNR]) {
#pragma unroll
        for (int i = 0; i < UNR; i++) {
            if constexpr (PRO == 0) {
                const int q = (tid + 256 * i) / (ROWS * 4);
                r[i].a = uok[i] ? *reinterpret_cast<const uint4*>(A.p[q < NP ? q : 0] + goff[i] + kc * 32) : make_uint4(0u, 0u, 0u, 0u);
            } else {
                const uint4 z = make_uint4(0u, 0u, 0u, 0u);
                r[i].a = uok[i] ? *reinterpret_cast<const uint4*>(Pf.X + goff[i] + kc * 32) : z;
                r[i].b = (uok[i] && Pf.S) ? *reinterpret_cast<const uint4*>(Pf.S + goff[i] + kc * 32) : z;
                if constexpr (PRO == 2) r[i].c = uok[i] ? *reinterpret_cast<const uint4*>(Pf.Y + goff[i] + kc * 32) : z;
            }
        }
    };
    auto stash = [&](int buf, int kc, const Raw (&r)[UNR]) {
#pragma unroll
        for (int i = 0; i < UNR; i++) {
            if constexpr (PRO == 0) {
                if (tid + 256 * i < NP * ROWS * 4) *reinterpret_cast<uint4*>(img + buf * NP * PB + loffs[i]) = r[i].a;
            } else {
                if (tid + 256 * i >= ROWS * 8) continue;
                const uint4& rc = PRO == 2 ? r[i].c : r[i].b;
                const float xa[4] = {__uint_as_float(r[i].a.x), __uint_as_float(r[i].a.y), __uint_as_float(r[i].a.z), __uint_as_float(r[i].a.w)};
                const float xb[4] = {__uint_as_float(r[i].b.x), __uint_as_float(r[i].b.y), __uint_as_float(r[i].b.z), __uint_as_float(r[i].b.w)};
                const float xc[4] = {__uint_as_float(rc.x), __uint_as_float(rc.y), __uint_as_float(rc.z), __uint_as_float(rc.w)};
                uint2 hi, lo;
                pro_operand<PRO>(Pf, ptab, kc * 32 + ((tid + 256 * i) & 7) * 4, goff[i] + kc * 32, uok[i], xa, xb, xc, hi, lo);
                if (!uok[i]) { hi = make_uint2(0u, 0u); lo = hi; }   // rows of a missing second board
                *reinterpret_cast<uint2*>(img + buf * NP * PB + loffs[i]) = hi;
                *reinterpret_cast<uint2*>(img + buf * NP * PB + PB + loffs[i]) = lo;
            }
        }
    };
    {
        Raw r0[UNR];
        fetch(0, r0);
        stash(0, 0, r0);
    }
    __syncthreads();
    // per lane: byte offset of its fragment row for (loop tap, tile) inside a part of a slice
    uint32_t arow[9][MT];
#pragma unroll
    for (int t = 0; t < 9; t++)
#pragma unroll
        for (int mt = 0; mt < MT; mt++) arow[t][mt] = (uint32_t)taprow[(AMODE == 2 ? 8 - t : t) * ZR + mt * 16 + c] * CHB + g * 16;

    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    s16x8 a[MT][NP];

    for (int kc = 0; kc < 8; kc++) {
        Raw nx[UNR];
        if (kc + 1 < 8) fetch(kc + 1, nx);
        const uint8_t* bufc = img + (kc & 1) * NP * PB;
        {   // the fragments of tap 0 of this slice (the slice became visible with the barrier that ended the previous chunk)
            constexpr uint32_t sk0 = skip_mask<NB>(AMODE == 2 ? 8 : 0);
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
                if (!((sk0 >> mt) & 1u))
#pragma unroll
                    for (int q = 0; q < NP; q++) a[mt][q] = *reinterpret_cast<const s16x8*>(bufc + q * PB + arow[0][mt]);
        }
        rs_tap<AMODE, NP, 0, F16>(bufc, kc, wsrc, loff, arow, bq, acc, a);
        rs_tap<AMODE, NP, 1, F16>(bufc, kc, wsrc, loff, arow, bq, acc, a);
        rs_tap<AMODE, NP, 2, F16>(bufc, kc, wsrc, loff, arow, bq, acc, a);
        rs_tap<AMODE, NP, 3, F16>(bufc, kc, wsrc, loff, arow, bq, acc, a);
        rs_tap<AMODE, NP, 4, F16>(bufc, kc, wsrc, loff, arow, bq, acc, a);
        rs_tap<AMODE, NP, 5, F16>(bufc, kc, wsrc, loff, arow, bq, acc, a);
        rs_tap<AMODE, NP, 6, F16>(bufc, kc, wsrc, loff, arow, bq, acc, a);
        rs_tap<AMODE, NP, 7, F16>(bufc, kc, wsrc, loff, arow, bq, acc, a);
        rs_tap<AMODE, NP, 8, F16>(bufc, kc, wsrc, loff, arow, bq, acc, a);
        if (kc + 1 < 8) stash((kc + 1) & 1, kc + 1, nx);
        __syncthreads();
    }
    // ---- C rows back in natural order: a lane holds 4 consecutive channels of one cell
    if constexpr (FUSE == 0 || FUSE == 2) {
        // FUSE = 2 (forward conv in training mode): + the batch-norm statistics of its own output (t_bn_stats: per channel sum and sum
        // of squares), per block of 2 boards, in double, cells of a lane first, then the 16 lanes of a channel group
        // -> F.part[blockIdx][2][256]
        double s[NT][4], ss[NT][4];
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
#pragma unroll
            for (int e = 0; e < 4; e++) s[nt][e] = ss[nt][e] = 0.0;
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            const int ci = rowcell[mt * 16 + c];
            if (ci == 0xffff || (ci >> 8) >= nbv) continue;
            float* out = C + (size_t)(m0 + (ci >> 8) * NPOS + (ci & 15) * 6 + ((ci >> 4) & 15)) * NF + wave * 64 + g * 4;
#pragma unroll
            for (int nt = 0; nt < NT; nt++) {
                if constexpr (F16) acc[mt][nt] *= oscale;
                *reinterpret_cast<float4*>(out + nt * 16) = make_float4(acc[mt][nt][0], acc[mt][nt][1], acc[mt][nt][2], acc[mt][nt][3]);
                if constexpr (FUSE == 2) {
#pragma unroll
                    for (int e = 0; e < 4; e++) bn_stat_fwd(acc[mt][nt][e], s[nt][e], ss[nt][e]);
                }
            }
        }
        if constexpr (FUSE == 2) {
#pragma unroll
            for (int nt = 0; nt < NT; nt++) part_butterfly_store(s[nt], ss[nt], c, F.part, blockIdx.x, wave * 64 + nt * 16 + g * 4);
        }
    } else {
        double s[NT][4], sx[NT][4];
        float4 mu[NT], is[NT];
#pragma unroll
        for (int nt = 0; nt < NT; nt++) {
            mu[nt] = *reinterpret_cast<const float4*>(F.mean + wave * 64 + g * 4 + nt * 16);
            is[nt] = *reinterpret_cast<const float4*>(F.istd + wave * 64 + g * 4 + nt * 16);
#pragma unroll
            for (int e = 0; e < 4; e++) s[nt][e] = sx[nt][e] = 0.0;
        }
        // EPG row tiles at a time: ALL their loads (shortcut gradient, post-activation, pre-BN output of layer l - 1 at the output
        // coordinates: up to 24 x 16 bytes per lane) are issued before the first is used — taken one tile at a time, every tile paid
        // its own round trip to memory (the weight ring and the fragment registers are dead here: the registers are free).
        // The sums run over the tiles in the same order as before: same bits.
        constexpr int EPG = 3;
        static_assert(MT % EPG == 0, "tiles per epilogue group");
#pragma unroll
        for (int m2 = 0; m2 < MT; m2 += EPG) {
            size_t o[EPG];
            bool valid[EPG];
            float4 d4[EPG][NT], a4[EPG][NT], y4[EPG][NT];
#pragma unroll
            for (int u = 0; u < EPG; u++) {
                const int mt = m2 + u;
                const int ci = rowcell[mt * 16 + c];
                valid[u] = !(ci == 0xffff || (ci >> 8) >= nbv);
                o[u] = (size_t)(m0 + (valid[u] ? (ci >> 8) * NPOS + (ci & 15) * 6 + ((ci >> 4) & 15) : 0)) * NF + wave * 64 + g * 4;
                if (valid[u]) {
#pragma unroll
                    for (int nt = 0; nt < NT; nt++) {
                        d4[u][nt] = F.DS ? *reinterpret_cast<const float4*>(F.DS + o[u] + nt * 16) : make_float4(0.f, 0.f, 0.f, 0.f);
                        a4[u][nt] = *reinterpret_cast<const float4*>(F.Apost + o[u] + nt * 16);
                        y4[u][nt] = *reinterpret_cast<const float4*>(F.Y + o[u] + nt * 16);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < EPG; u++) {
                const int mt = m2 + u;
                if (valid[u]) {
#pragma unroll
                    for (int nt = 0; nt < NT; nt++) {
                        float4 v = make_float4(acc[mt][nt][0], acc[mt][nt][1], acc[mt][nt][2], acc[mt][nt][3]);
                        if (F.DS) { v.x += d4[u][nt].x; v.y += d4[u][nt].y; v.z += d4[u][nt].z; v.w += d4[u][nt].w; }
                        *reinterpret_cast<float4*>(C + o[u] + nt * 16) = v;
                        const float vv[4] = {v.x, v.y, v.z, v.w}, aa[4] = {a4[u][nt].x, a4[u][nt].y, a4[u][nt].z, a4[u][nt].w},
                                    yy[4] = {y4[u][nt].x, y4[u][nt].y, y4[u][nt].z, y4[u][nt].w};
                        const float mm[4] = {mu[nt].x, mu[nt].y, mu[nt].z, mu[nt].w}, ii[4] = {is[nt].x, is[nt].y, is[nt].z, is[nt].w};
#pragma unroll
                        for (int e = 0; e < 4; e++) bn_stat_bwd(aa[e] > 0.0f ? vv[e] : 0.0f, yy[e], mm[e], ii[e], s[nt][e], sx[nt][e]);
                    }
                }
            }
        }
#pragma unroll
        for (int nt = 0; nt < NT; nt++) part_butterfly_store(s[nt], sx[nt], c, F.part, blockIdx.x, wave * 64 + nt * 16 + g * 4);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// t_conv_q: the same conv GEMMs for SMALL batches — a rank's 64-record share of a data-parallel minibatch, or a small
// minibatch.  t_conv_rs gives a CU 2 boards x 256 channels: 32 blocks at 64 records, an eighth of the chip, and the kernel takes
// as long as for 512 records (a block's serial work sets the time).  Here a block is ONE board x 64 output channels
// (blockIdx = board * 4 + channel group: 256 blocks at 64 records), and its 4 waves split K: wave w owns the 32-channel slices
// w and w + 4 of the board (2 x 9 k-steps), staged privately by the wave itself (no barrier until the end), its partial sums
// [48 rows x 64 channels] meet the other three waves' in LDS and are added in wave order (fixed: bit-reproducible); wave w
// then finishes column tile w (16 channels): store, and the same epilogue / staging-path fusions as t_conv_rs (FUSE, PRO;
// the side outputs of PRO are written by channel group 0 only).  One board = rows in natural order, 3 row tiles, no skipped
// (tile, tap) pairs.  Operands: two parts (fp16 pair with F16, else bf16 hi / mid), 3 passes.
// ---------------------------------------------------------------------------------------------------------------------
struct Rq {
    static constexpr int ROWS = 42, MT = 3, ZR = 48, NT = 4, RING = 3, NP = 2;
    static constexpr int CHB = 80;                       // bytes per row of a 32-channel slice (64 + 16 pad)
    static constexpr int PB = (ZR + 1) * CHB;            // one part of one slice, incl. the zero row
    static constexpr int WIMG = 2 * NP * PB;             // a wave's two slices
    static constexpr int RED = 4 * MT * NT * 64 * 16;    // the four waves' partial sums (f32x4 per lane)
    static constexpr int LDS = (4 * WIMG > RED ? 4 * WIMG : RED);
};

template <int AMODE, int FUSE, bool F16, int PRO>
__global__ __launch_bounds__(256, 1) void t_conv_q(Parts A, Parts Bp, float* __restrict__ C, int boards, BwdFuse F, float oscale, ProFuse Pf)
{
    constexpr int ROWS = Rq::ROWS, MT = Rq::MT, ZR = Rq::ZR, NT = Rq::NT, RING = Rq::RING, NP = Rq::NP, CHB = Rq::CHB, PB = Rq::PB;
    constexpr uint32_t KB = Rs::KB;
    __shared__ __attribute__((aligned(16))) uint8_t img[Rq::LDS];
    __shared__ uint8_t taprow[9 * ZR];
    __shared__ __attribute__((aligned(16))) float ptab[PRO ? 5 * NF : 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    // (wave enters the weight loads' scalar offset and the compiler cannot prove it wave-uniform: each of those loads sits in a waterfall loop.
    //  Saying so with readfirstlane removes the loops and 32 VGPRs — and measures SLOWER at 64 records: 43.7 / 25.4 us against 34.6 / 20.2 for
    //  the backward / forward conv; the loops pace the loads between the MFMAs better than the scheduler does without them.  Left as it is.)
    const int board = blockIdx.x >> 2, cq = blockIdx.x & 3, m0 = board * NPOS;
    (void)boards;

    // ---- weight ring: this wave's first two k-steps (slice `wave`, taps 0 and 1) fly while the tables are built
    __amdgpu_buffer_rsrc_t wsrc[NP];
#pragma unroll
    for (int q = 0; q < NP; q++) wsrc[q] = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(Bp.p[q]), (short)0, (int)(WPACK * 2), 0x00020000);
    const uint32_t loff = (uint32_t)((cq * NT) * 64 + lane) * 16u;
    u32x4 bq[RING][NP][NT];
    auto kstep_off = [&](int s2) { return (uint32_t)((s2 % 9) * 8 + wave + 4 * (s2 / 9)) * KB; };   // k-step s2 of this wave: tap s2 % 9 of slice wave + 4 (s2 / 9)
#pragma unroll
    for (int s2 = 0; s2 < RING - 1; s2++)
#pragma unroll
        for (int q = 0; q < NP; q++)
#pragma unroll
            for (int nt = 0; nt < NT; nt++) bq[s2][q][nt] = __builtin_amdgcn_raw_buffer_load_b128(wsrc[q], loff + nt * 1024, (int)kstep_off(s2), 0);

    // ---- tables: source row of (geometric tap, row); pad rows and out-of-board taps read the zero row
    for (int i = tid; i < 9 * ZR; i += 256) {
        const int t = i / ZR, r = i - t * ZR;
        int src = ZR;
        if (r < ROWS) {
            const int y = r / 6 + t / 3 - 1, x = r % 6 + t % 3 - 1;
            if ((unsigned)y < 7u && (unsigned)x < 6u) src = y * 6 + x;
        }
        taprow[i] = (uint8_t)src;
    }
    if constexpr (PRO != 0) ptab_fill<PRO>(Pf, ptab, tid);
    uint8_t* wimg = img + wave * Rq::WIMG;   // this wave's two slices: [slice][part][row][80 B]
    for (int i = lane; i < 2 * NP * (CHB / 4); i += 64) {   // their zero rows
        const int sp = i / (CHB / 4), w4 = i % (CHB / 4);
        reinterpret_cast<uint32_t*>(wimg + sp * PB + ZR * CHB)[w4] = 0u;
    }
    __syncthreads();

    // ---- the wave stages its two 32-channel slices itself (kc = wave, wave + 4)
#pragma unroll
    for (int sl = 0; sl < 2; sl++) {
        const int kc = wave + 4 * sl;
        uint8_t* dst = wimg + sl * NP * PB;
        if constexpr (PRO == 0) {
            constexpr int UNITS = NP * ROWS * 4;   // (part, row, 16-byte segment)
#pragma unroll
            for (int i = 0; i < (UNITS + 63) / 64; i++) {
                const int u = lane + 64 * i;
                if (u < UNITS) {
                    const int q = u / (ROWS * 4), rem = u - q * (ROWS * 4), r = rem >> 2, seg = rem & 3;
                    *reinterpret_cast<uint4*>(dst + q * PB + r * CHB + seg * 16) =
                        *reinterpret_cast<const uint4*>(A.p[q] + (size_t)(m0 + r) * NF + kc * 32 + seg * 8);
                }
            }
        } else {
            constexpr int UNITS = ROWS * 8;        // (row, 4 channels)
#pragma unroll
            for (int i = 0; i < (UNITS + 63) / 64; i++) {
                const int u = lane + 64 * i;
                if (u >= UNITS) continue;
                const int r = u >> 3, seg = u & 7, ch = kc * 32 + seg * 4;
                const size_t go = (size_t)(m0 + r) * NF + ch;
                const float4 xa4 = *reinterpret_cast<const float4*>(Pf.X + go);
                const float4 xb4 = Pf.S ? *reinterpret_cast<const float4*>(Pf.S + go) : make_float4(0.f, 0.f, 0.f, 0.f);
                const float4 xc4 = PRO == 2 ? *reinterpret_cast<const float4*>(Pf.Y + go) : xb4;
                const float xa[4] = {xa4.x, xa4.y, xa4.z, xa4.w}, xb[4] = {xb4.x, xb4.y, xb4.z, xb4.w}, xc[4] = {xc4.x, xc4.y, xc4.z, xc4.w};
                uint2 hi, lo;
                pro_operand<PRO>(Pf, ptab, ch, go, cq == 0, xa, xb, xc, hi, lo);
                *reinterpret_cast<uint2*>(dst + r * CHB + seg * 8) = hi;
                *reinterpret_cast<uint2*>(dst + PB + r * CHB + seg * 8) = lo;
            }
        }
    }
    asm volatile("" ::: "memory");   // (a wave's LDS operations execute in program order: its fragment reads follow its own stores)

    // per lane: byte offset of its fragment row for (loop tap, tile) inside a part of a slice
    uint32_t arow[9][MT];
#pragma unroll
    for (int t = 0; t < 9; t++)
#pragma unroll
        for (int mt = 0; mt < MT; mt++) arow[t][mt] = (uint32_t)taprow[(AMODE == 2 ? 8 - t : t) * ZR + mt * 16 + c] * CHB + g * 16;

    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    s16x8 a[MT][NP];
#pragma unroll
    for (int s2 = 0; s2 < 18; s2++) {
        const int sl = s2 / 9, t = s2 % 9, cur = s2 % RING, ref = (s2 + RING - 1) % RING;
        const uint8_t* bufc = wimg + sl * NP * PB;
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int q = 0; q < NP; q++) a[mt][q] = *reinterpret_cast<const s16x8*>(bufc + q * PB + arow[t][mt]);
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
#pragma unroll
            for (int p = 0; p < 3; p++) {
                const int qa = RsPass<2>::QA[p], qb = RsPass<2>::QB[p];
#pragma unroll
                for (int nt = 0; nt < NT; nt++) acc[mt][nt] = mfma_part<F16>(bq[cur][qb][nt], a[mt][qa], acc[mt][nt]);
                // one refill load of the ring slot the previous k-step freed per pass (8 loads over the 9 passes of a k-step)
                const int slot = mt * 3 + p;
                if (slot < NP * NT && s2 + RING - 1 < 18)
                    bq[ref][slot / NT][slot % NT] = __builtin_amdgcn_raw_buffer_load_b128(wsrc[slot / NT], loff + (slot % NT) * 1024, (int)kstep_off(s2 + RING - 1), 0);
            }
        }
    }

    // ---- the four waves' partial sums meet in LDS (over the slices: every wave is done reading), added in wave order
    __syncthreads();
    f32x4* red = reinterpret_cast<f32x4*>(img);
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) red[((wave * MT + mt) * NT + nt) * 64 + lane] = acc[mt][nt];
    __syncthreads();
    f32x4 out[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        out[mt] = red[((0 * MT + mt) * NT + wave) * 64 + lane];
#pragma unroll
        for (int w = 1; w < 4; w++) out[mt] += red[((w * MT + mt) * NT + wave) * 64 + lane];
        if constexpr (F16) out[mt] *= oscale;
    }
    // wave w holds column tile w: lane (c, g) = cell mt * 16 + c, channels cq * 64 + wave * 16 + g * 4 ..
    const int ch0 = cq * 64 + wave * 16 + g * 4;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, sx[4] = {0.0, 0.0, 0.0, 0.0};
    float4 mu4 = make_float4(0.f, 0.f, 0.f, 0.f), is4 = mu4;
    if constexpr (FUSE == 1) { mu4 = *reinterpret_cast<const float4*>(F.mean + ch0); is4 = *reinterpret_cast<const float4*>(F.istd + ch0); }
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        const int r = mt * 16 + c;
        if (r >= ROWS) continue;
        const size_t o = (size_t)(m0 + r) * NF + ch0;
        float4 v = make_float4(out[mt][0], out[mt][1], out[mt][2], out[mt][3]);
        if constexpr (FUSE == 1) {
            if (F.DS) {
                const float4 d = *reinterpret_cast<const float4*>(F.DS + o);
                v.x += d.x; v.y += d.y; v.z += d.z; v.w += d.w;
            }
        }
        *reinterpret_cast<float4*>(C + o) = v;
        const float vv[4] = {v.x, v.y, v.z, v.w};
        if constexpr (FUSE == 2) {
#pragma unroll
            for (int e = 0; e < 4; e++) bn_stat_fwd(vv[e], s[e], sx[e]);
        } else if constexpr (FUSE == 1) {
            const float4 a4 = *reinterpret_cast<const float4*>(F.Apost + o), y4 = *reinterpret_cast<const float4*>(F.Y + o);
            const float aa[4] = {a4.x, a4.y, a4.z, a4.w}, yy[4] = {y4.x, y4.y, y4.z, y4.w};
            const float mm[4] = {mu4.x, mu4.y, mu4.z, mu4.w}, ii[4] = {is4.x, is4.y, is4.z, is4.w};
#pragma unroll
            for (int e = 0; e < 4; e++) bn_stat_bwd(aa[e] > 0.0f ? vv[e] : 0.0f, yy[e], mm[e], ii[e], s[e], sx[e]);
        }
    }
    if constexpr (FUSE != 0) {   // per-channel partials of this board: cells of a lane, then the 16 lanes of a channel group
        part_butterfly_store(s, sx, c, F.part, board, ch0);
    }
}

}  // namespace
