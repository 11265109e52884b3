// azr_train.hip — the optimiser step of the learn loop on the GPU (SURVEY §8 f-2, C-ABI azr_nn_train*).
//
// Replaces AlphaZeroNN::train (neural_network/alphazero_nn.cpp:351-410), i.e. `session->Run({state, target pi, target v,
// training=true}, {loss_policy, loss_value}, {optimize})` on the graph of python/src/build_graph.py:54-103:
//   forward in training mode (batch-statistics BN, moving averages updated with momentum 0.99), loss =
//   softmax-CE(pi) + MSE(v) + 1e-3 * sum ||kernel||^2, backward, Adam(1e-3, .9, .999, 1e-8) — all fp32 like the
//   reference's TF session.
//
// Data layout (all fp32, row-major): an activation is [M = batch * 42 rows][256 channels], row = board * 42 + y * 6 + x —
// the inference kernels' row order.  A 3x3 SAME convolution is the implicit GEMM  im2col(A) [M][9 * 256]  x  W [9 * 256][256]
// (W = the AZRW kernel [tap][ci][co] as it lies in the flat vector); the im2col matrix is never materialised — the tile
// loader gathers the shifted rows.  Its two gradients are the same kernel with other operand views: dW = im2col(A)^T x
// dY (split-K), dA = im2col-(dY) x W^T (negated taps).  Arithmetic: split bf16 on v_mfma_f32_16x16x32_bf16 — an fp32
// value is the exact sum of three bf16 parts; the forward multiplies all parts that matter (6 MFMA passes, fp32-exact
// products, so ReLU masks and batch statistics are those of an fp32 forward), the two gradient GEMMs use two parts (3
// passes, 1e-5 relative) — with t_gemm on the fp32 MFMA (v_mfma_f32_32x32x2_f32) kept for the stem (K = 144), odd
// batch sizes and AZR_TRAIN_GEMM=f32.  Kernels of the split path: t_conv_rs / t_conv_q (forward on fp16 pairs, backward-data on two
// bf16 parts, with the normalise and statistics steps fused into their staging paths and epilogues) and t_wgrad_g5 (weight gradient).
// Every conv output (pre-BN) and every post-activation is kept for the backward pass: 2 x 22 MB per layer at batch 512,
// 1.8 GB for the 41 conv layers of B = 20 — sized for 288 GB of HBM, nothing is recomputed.
// Reductions (BN statistics, bias / BN / head gradients, split-K) are two-stage and atomic-free: a step is
// bit-reproducible.
// This file is the host side — training context, step, validation pass, C-ABI — and the small one-off kernels; the kernel families are in
// the headers it includes (one translation unit): azr_train_conv.hpp (split / pack helpers, the batch-norm arithmetic stated once,
// t_conv_rs, t_conv_q), azr_train_wgrad.hpp (t_wgrad_g5, slice sums), azr_train_bn.hpp (batch-norm and head kernels), azr_train_gemm.hpp.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <rccl/rccl.h>   // types and enumerators only: the library is bound at run time (rccl_api below)
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "azr_internal.hpp"
#include "azr_train_bn.hpp"
#include "azr_train_conv.hpp"
#include "azr_train_gemm.hpp"
#include "azr_train_wgrad.hpp"

using namespace azr;

namespace {

// =====================================================================================================================
// data movement
// =====================================================================================================================
// records [n][265] (i8 player | in88 | f32 z | f32 pi[43]; alphazero_nn_data.h:111-141) -> minibatch tensors
// `cur` = {offset of this minibatch in perm, Adam step count}: device-resident so that one captured graph serves every step
__global__ void t_gather(const uint8_t* __restrict__ rec, const int* __restrict__ perm, const int* __restrict__ cur, int BS,
                         uint8_t* __restrict__ in88, float* __restrict__ pit, float* __restrict__ zt)
{
    const int b = blockIdx.x, t = threadIdx.x;
    const uint8_t* r = rec + (size_t)perm[cur[0] + cur[2] + b] * 265;   // cur[2] = this rank's offset inside the global minibatch
    for (int i = t; i < 88; i += blockDim.x) in88[b * 88 + i] = r[1 + i];
    for (int i = t; i < 44; i += blockDim.x) {
        float f;
        memcpy(&f, r + 89 + 4 * i, 4);
        if (i == 0) zt[b] = f; else pit[b * 43 + i - 1] = f;
    }
}

// setInStateTensor (alphazero_nn.cpp:31-67): in88 -> [M][16] planes (13 used)
__global__ void t_planes(const uint8_t* __restrict__ in88, int M, float* __restrict__ X0)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * SIN) return;
    const int r = i / SIN, c = i % SIN, b = r / NPOS, pos = r % NPOS;
    const uint8_t* in = in88 + (size_t)b * 88;
    float v = 0.0f;
    if (c < 13) {
        const uint32_t la = in[pos];
        const int army = la & 63, owner = la >> 6, cur = in[42], enemy = cur == 0 ? 1 : 0;
        const float fa = (float)army / 32.0f;
        float f[10];
        memcpy(f, in + 48, 40);
        switch (c) {
        case 0: v = owner == cur ? fa : 0.0f; break;
        case 1: v = owner == enemy ? fa : 0.0f; break;
        case 2: v = owner == 2 ? fa : 0.0f; break;
        case 3: v = f[9]; break;
        case 4: v = f[0]; break;
        case 5: v = f[1]; break;
        case 6: v = f[2]; break;
        default: v = f[3 + (c - 7)]; break;
        }
    }
    X0[i] = v;
}

// stem kernel [9][13][256] <-> padded [9][16][256]
__global__ void t_stem_pad(const float* __restrict__ w, float* __restrict__ wp)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= KS * NF) return;
    const int co = i % NF, ci = (i / NF) % SIN, tap = i / (NF * SIN);
    wp[i] = ci < 13 ? w[((size_t)tap * 13 + ci) * NF + co] : 0.0f;
}
__global__ void t_stem_unpad(const float* __restrict__ gp, float* __restrict__ g)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 9 * 13 * NF) return;
    const int co = i % NF, ci = (i / NF) % 13, tap = i / (NF * 13);
    g[i] = gp[((size_t)tap * SIN + ci) * NF + co];
}

// col[r][tap][c] = A[r + dy*6 + dx][c] inside the board, else 0   (tap = (dy+1)*3 + (dx+1))
template <int C>
__global__ __launch_bounds__(256) void t_im2col(const float* __restrict__ A, float* __restrict__ col, int M)
{
    const int idx = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (idx >= M * 9) return;
    const int r = idx / 9, tap = idx % 9, dy = tap / 3 - 1, dx = tap % 3 - 1;
    const int pos = r % NPOS, y = pos / 6 + dy, x = pos % 6 + dx;
    const bool ok = y >= 0 && y < 7 && x >= 0 && x < 6;
    const float4* src = reinterpret_cast<const float4*>(A) + (size_t)(r + dy * 6 + dx) * (C / 4);
    float4* dst = reinterpret_cast<float4*>(col) + (size_t)idx * (C / 4);
    for (int q = lane; q < C / 4; q += 64) dst[q] = ok ? src[q] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// a += b
__global__ __launch_bounds__(256) void t_add(float* __restrict__ a, const float* __restrict__ b, size_t n4)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float4 x = reinterpret_cast<float4*>(a)[i];
    const float4 y = reinterpret_cast<const float4*>(b)[i];
    x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w;
    reinterpret_cast<float4*>(a)[i] = x;
}

// =====================================================================================================================
// Adam (tf.train.AdamOptimizer: lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t); w -= lr_t * m / (sqrt(v) + eps)); kind 1 adds
// the L2 regulariser's gradient 2 * L2_C * w (keras l2 = l * sum w^2), kind 0 (BN moving statistics) is not trained
// =====================================================================================================================
// step t := t + 1 and its bias-corrected learning rate; afterwards the minibatch offset advances
__global__ void t_tick_lr(int* __restrict__ cur, float* __restrict__ lr)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double t = (double)(++cur[1]);
    *lr = (float)((double)LR * sqrt(1.0 - pow((double)ADAM_B2, t)) / (1.0 - pow((double)ADAM_B1, t)));
}
__global__ void t_tick_batch(int* __restrict__ cur, int BS /* the GLOBAL minibatch */)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) cur[0] += BS;
}

__global__ void t_adam(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                       const uint8_t* __restrict__ kind, size_t n, const float* __restrict__ lr)
{
    const float lr_t = *lr;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int k = kind[i];
    if (k == 0) return;
    float gi = g[i];
    if (k == 1) gi += 2.0f * L2_C * w[i];
    const float mi = ADAM_B1 * m[i] + (1.0f - ADAM_B1) * gi;
    const float vi = ADAM_B2 * v[i] + (1.0f - ADAM_B2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    w[i] -= lr_t * mi / (sqrtf(vi) + ADAM_EPS);
}

// =====================================================================================================================
// The step with options (azr_nn_train_set_options; formulae in include/azr.h).  With every option at its default the step
// launches t_tick_lr and t_adam above and none of these; with neutral options (lr = LR, l2 = L2_C, s = 1) these give the
// same bits: the arithmetic below is t_tick_lr's and t_adam's, with factors that are exactly 1.
// =====================================================================================================================
// what the kernels leave for azr_nn_train_stats: one row in device memory, so that azr_nn_train's queue of steps never waits for the host
struct StatRow {
    float lr;            // t_tick_lr_sched: the scheduled rate lr_eff of the last step
    float norm;          // t_grad_sqsum_final: the global gradient norm (t_tick_lr_sched: NaN while clipping is off)
    float scale;         // ... and the clip scale s that t_adam_opt multiplies by (1 while clipping is off)
    int pad;
    long long clipped;   // steps with s < 1 since the optimiser state was created
};
struct Sched {
    double lr, r, gamma;   // base rate, lr_min / lr, STEP's factor
    int schedule, W, N, period;
    int clip;              // clipping is on: t_grad_sqsum_final has written norm and scale
};

__global__ void t_tick_lr_sched(int* __restrict__ cur, float* __restrict__ lr, StatRow* __restrict__ row, Sched a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int ti = ++cur[1];
    const double t = (double)ti;
    const double warm = a.W > 0 ? fmin(1.0, t / (double)a.W) : 1.0;
    double f = 1.0;
    if (a.schedule == AZR_LR_COSINE) {
        const double p = fmin(1.0, fmax(0.0, (t - (double)a.W) / (double)(a.N - a.W)));
        f = a.r + (1.0 - a.r) * 0.5 * (1.0 + cos(M_PI * p));
    } else if (a.schedule == AZR_LR_STEP) {
        f = pow(a.gamma, (double)((ti - 1) / a.period));
    }
    const double lr_eff = a.lr * warm * f;
    *lr = (float)(lr_eff * sqrt(1.0 - pow((double)ADAM_B2, t)) / (1.0 - pow((double)ADAM_B1, t)));
    row->lr = (float)lr_eff;
    if (!a.clip) { row->norm = __builtin_nanf(""); row->scale = 1.0f; }
}

// sum of g^ ^2 over the trained slots, g^ in fp32 as t_adam_opt forms it, squares and sums in double.  A FIXED grid (the order of the
// partials does not depend on the device): thread j of SQ_BLOCKS * 256 takes slots j, j + SQ_BLOCKS * 256, ...; its sum goes
// down the wavefront by cross-lane moves (32, 16, ... 1), the block's four wave sums through LDS, in wave order -> part[block].
constexpr int SQ_BLOCKS = 1024;
__global__ __launch_bounds__(256) void t_grad_sqsum(const float* __restrict__ w, const float* __restrict__ g, const uint8_t* __restrict__ kind,
                                                    size_t n, float l2x2, double* __restrict__ part)
{
    __shared__ double ws[4];
    constexpr size_t SWEEP = (size_t)SQ_BLOCKS * 256;
    auto sq = [l2x2](int k, float gi, float wi) {
        if (k == 1) gi += l2x2 * wi;
        return k == 0 ? 0.0 : (double)gi * (double)gi;
    };
    double acc = 0.0;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    // four sweeps per trip: twelve loads in flight per lane, the squares added in slot order as the one-sweep loop below adds them
    for (; i + 3 * SWEEP < n; i += 4 * SWEEP) {
        const int k0 = kind[i], k1 = kind[i + SWEEP], k2 = kind[i + 2 * SWEEP], k3 = kind[i + 3 * SWEEP];
        const float g0 = g[i], g1 = g[i + SWEEP], g2 = g[i + 2 * SWEEP], g3 = g[i + 3 * SWEEP];
        const float w0 = w[i], w1 = w[i + SWEEP], w2 = w[i + 2 * SWEEP], w3 = w[i + 3 * SWEEP];
        acc += sq(k0, g0, w0);
        acc += sq(k1, g1, w1);
        acc += sq(k2, g2, w2);
        acc += sq(k3, g3, w3);
    }
    for (; i < n; i += SWEEP) acc += sq(kind[i], g[i], w[i]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}
// one block: the partials in index order -> norm, s = clip / max(norm, clip), the count of clipped steps
__global__ __launch_bounds__(256) void t_grad_sqsum_final(const double* __restrict__ part, double clip, StatRow* __restrict__ row)
{
    __shared__ double ps[SQ_BLOCKS];
    for (int i = threadIdx.x; i < SQ_BLOCKS; i += 256) ps[i] = part[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sum = 0.0;
    for (int i = 0; i < SQ_BLOCKS; i++) sum += ps[i];
    const double norm = sqrt(sum);
    const float s = (float)(clip / fmax(norm, clip));
    row->norm = (float)norm;
    row->scale = s;
    if (s < 1.0f) row->clipped += 1;
}

// t_adam on s * g^ at the scheduled rate, and the EMA of the new weights in the same pass (no second sweep over the vectors)
template <bool EMA>
__global__ void t_adam_opt(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, float* __restrict__ e,
                           const uint8_t* __restrict__ kind, size_t n, const float* __restrict__ lr, const StatRow* __restrict__ row, float l2x2,
                           float d)
{
    const float lr_t = *lr, s = row->scale;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int k = kind[i];
    if (k == 0) {   // BN moving statistics: the forward pass of this step has updated them, and they are averages already
        if (EMA) e[i] = w[i];
        return;
    }
    float wi = w[i];
    float gi = g[i];
    if (k == 1) gi += l2x2 * wi;
    gi *= s;
    const float mi = ADAM_B1 * m[i] + (1.0f - ADAM_B1) * gi;
    const float vi = ADAM_B2 * v[i] + (1.0f - ADAM_B2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    wi -= lr_t * mi / (sqrtf(vi) + ADAM_EPS);
    w[i] = wi;
    if (EMA) e[i] = d * e[i] + (1.0f - d) * wi;
}

// =====================================================================================================================
// host
// =====================================================================================================================
// conv GEMM arithmetic: split bf16 (default; 6-pass forward, 3-pass backward) or the fp32 MFMA (AZR_TRAIN_GEMM=f32)
// (all five are test hooks: run-time switches in libazr_hip_test.so, compile-time constants in the product library)
#ifdef AZR_TEST_HOOKS
#define AZR_HOOK_FLAG bool
#else
#define AZR_HOOK_FLAG constexpr bool
#endif
AZR_HOOK_FLAG g_gemm_bf16x3 = true;
// forward conv arithmetic: fp16 pairs, 3 passes (default) or three bf16 parts, 6 passes (AZR_TRAIN_FWD=bf16)
AZR_HOOK_FLAG g_fwd_f16 = true;
constexpr float FWD_WSCALE = 1024.0f;   // the packed forward kernels are 2^10 * W: |w| < 64 stays inside fp16, a weight of 1e-4 keeps a normal low part
AZR_HOOK_FLAG g_fuse_bwd = true;
#ifndef WG5_NC
#define WG5_NC 4   // co tiles per wave of t_wgrad_g5 (2: half the split-K partials but 20 fragment reads per 54 MFMAs instead of 28 per 108 — 86.9 us against 61.2)
#endif
AZR_HOOK_FLAG g_wgrad_g5 = true;    // t_wgrad_g5 (k-step = a board row of five boards); AZR_TRAIN_WGRAD=rs: t_wgrad_rs (rows in memory order), the older formulation
AZR_HOOK_FLAG g_conv_q = true;       // t_conv_q for batches of up to 128 records (AZR_TRAIN_CONVQ=0: t_conv_rs at every size)
// g_fuse_bwd (declared above): t_conv_rs<2, 2, 1>: shortcut add + BN-backward stage 1 in the backward-data conv's epilogue, and the batch
// statistics in the forward conv's (AZR_TRAIN_FUSE=0: separate kernels)
// t_conv_rs<.., PRO>: the normalise kernels (t_bn_apply / t_bn_bwd_apply) computed in the consuming conv's staging path
// (AZR_TRAIN_FUSE_APPLY=0: separate kernels; same bits)
AZR_HOOK_FLAG g_fuse_apply = true;


// The kernel choice of the step, derived once per set of slabs (ctx_ensure: the hooks are read and the batch size is known there);
// everything below ctx_ensure reads the plan and no switch.
struct Plan {
    bool sb = false;      // split-bf16 conv GEMMs (the stem, K = 144, and row counts that are no multiple of the k-tile stay on the fp32 MFMA)
    bool f16 = false;     // forward conv: fp16 pairs, 3 passes
    bool fap = false;     // layer l's normalise step is computed in the staging path of the forward conv of layer l + 1
    bool convq = false;   // small batches (a rank's share of a data-parallel minibatch): t_conv_q, one board x 64 channels per block
    bool wg5 = true;      // weight gradient: t_wgrad_g5 (the hook's other choice: t_wgrad_rs)
    bool fuse = false;    // split path: batch statistics in the forward conv's epilogue, BN-backward stage 1 in the backward-data conv's
    bool bap = false;     // ... and t_bn_bwd_apply computed in the backward-data conv's staging path: the product's backward pass
};

// ---- Two lifetimes.  Slabs: everything sized by the batch (BS / M / R / nz / wg_*), with those numbers and the plan; freed and rebuilt
// when a call comes with another batch size (a validation pass behind a training step, data-parallel shares of another size).
// TrainState: the optimiser state and everything sized by the net's depth alone; one per handle, created by the first training or
// validation call, freed by azr_nn_train_reset, a failed health check and engine destroy.  A rebuild of the slabs never touches it.
struct Slabs {
    int BS = 0, M = 0, R = 0, nz = 0, kchunk = 0;
    Plan plan;
    int wg_slices = 0;                       // weight gradient: slices (split-K units of whole boards)
    int wg_bps = 0;                          // ... boards per slice
    int wg_parts = 0;                        // ... split-K partials that reach memory (t_wgrad_g5: one per four slices, summed in the block)
    float *X0 = nullptr, *col0 = nullptr;
    float *Y = nullptr, *A = nullptr;        // [L][M][256]
    float *G = nullptr, *DS = nullptr, *DT = nullptr, *dY = nullptr;
    double* part = nullptr;                  // [R][2*NG][256]
    float* wpart = nullptr;                  // split-K partials [nz][KC][256]
    uint16_t *ap[3] = {nullptr, nullptr, nullptr}, *dyp[2] = {nullptr, nullptr};          // bf16 parts of activations / gradients
    uint16_t* dyp2[2] = {nullptr, nullptr};  // the dY parts of odd layers (a second set: the chain runs ahead of the weight-gradient branch)
    uint16_t* af[2] = {nullptr, nullptr};    // fp16 pair (hi, lo) of the newest post-activation: the next forward conv's operand
    float *pv0 = nullptr, *dpv = nullptr, *fpi = nullptr, *fv = nullptr, *h1 = nullptr, *vout = nullptr, *prob = nullptr, *lossb = nullptr,
          *hpart = nullptr, *cpart = nullptr;
    uint8_t* in88 = nullptr;
    float *pit = nullptr, *zt = nullptr;
    std::vector<void*> allocs;

    ~Slabs() { for (void* p : allocs) hipFree(p); }   // (held by a unique_ptr, never copied)
    // views of layer l: pre-BN conv output, post-activation and its bf16 parts (the third part only until the next forward conv has read it)
    size_t act() const { return (size_t)M * NF; }
    float* Yl(int l) const { return Y + act() * l; }
    float* Al(int l) const { return A + act() * l; }
    Parts Ap(int l) const { return Parts{{ap[0] + act() * l, ap[1] + act() * l, ap[2]}}; }
};

// data-parallel step (azr_nn_train_dp): this rank's shard of every minibatch; sums that span the batch are all-reduced.  A call sets
// the link and resets it by assignment (a data-parallel call that failed half-way must not linger).
struct DpLink {
    int world = 1, rank = 0;
    azr_allreduce_fn ar = nullptr;
    void* ar_ctx = nullptr;
    bool native = false;       // the sums go through the handle's own RCCL communicator, in stream order (azr_dp_init)
    // the data-parallel code path (a callback was supplied, or the handle has a communicator), also with one rank
    bool dp() const { return ar != nullptr || native; }
};

// the device cursor `cur` of t_gather, the tick kernels and t_pack_w (the kernels index it as an int*)
enum { CUR_OFFSET = 0, CUR_STEP = 1, CUR_RANK = 2, CUR_RANGE = 3, CUR_N = 4 };   // minibatch offset in perm, Adam step count, this rank's offset inside the minibatch, range flag

struct TrainState {
    int blocks = 0, L = 0;
    size_t count = 0;
    long step = 0;
    float *g = nullptr, *m = nullptr, *v = nullptr;   // g: cleared once, here — the slots the backward pass never writes stay 0
    uint8_t* kind = nullptr;
    float *wpad = nullptr, *gpad = nullptr;
    float *mean = nullptr, *istd = nullptr;  // [L][256]
    float* sums = nullptr;                   // [2][256]
    uint16_t *wpf[3] = {nullptr, nullptr, nullptr}, *wpb[2] = {nullptr, nullptr};        // packed kernels: forward / backward-data view
    float *hstat = nullptr, *loss = nullptr;
    int* cur = nullptr;        // device: [CUR_N]
    DpLink link;
    double* red = nullptr;     // [2 * NG][256] reduced BN partials
    double* hsum = nullptr;    // [6] head BN sums
    float* lr = nullptr;   // device: this step's bias-corrected learning rate
    // the step's options (azr_nn_train_set_options), copied from the handle when a training call is entered
    azr_train_options opt = {};
    bool opt_default = true;     // ... every one at its default: the step launches t_tick_lr and t_adam
    bool last_default = true;    // the path the LAST step took (azr_nn_train_stats)
    StatRow* row = nullptr;      // device: what the step's kernels leave for azr_nn_train_stats
    double* sqpart = nullptr;    // device: [SQ_BLOCKS] partial sums of the gradient norm
    float* e = nullptr;          // device: the EMA vector, created by the first step with ema_decay > 0; optimiser state like m and v
    long ema_steps = 0;          // steps folded into it
    // the weight-gradient branch of the backward pass (t_wgrad_g5 + t_sum_slices of every layer) hangs off the gradient chain: nothing
    // but Adam waits for it.  At small batches (<= 128 records: a rank's share of a data-parallel minibatch) it runs on a second,
    // low-priority stream beside the chain's kernels, which leave most of the chip idle there: 4.22 -> 3.87 ms per step at 64 records.
    hipStream_t side = nullptr;
    hipEvent_t ev_conv[2] = {nullptr, nullptr};   // main -> side: the backward-data conv of a layer has left its dY parts (by layer parity)
    hipEvent_t ev_wg[2] = {nullptr, nullptr};     // side -> main: that layer's weight gradient has read them
    // grow-only (grow): the call's records and their order, and the validation pass's buffer (ValHdr)
    uint8_t* rec = nullptr;
    int* perm = nullptr;
    float* vbuf = nullptr;
    size_t rec_cap = 0, perm_cap = 0, vbuf_cap = 0;
    std::vector<void*> allocs;
    std::unique_ptr<Slabs> slabs;   // null until the first call, and behind a rebuild that failed: the next call rebuilds

    ~TrainState()
    {
        slabs.reset();
        for (int q = 0; q < 2; q++) { if (ev_conv[q]) hipEventDestroy(ev_conv[q]); if (ev_wg[q]) hipEventDestroy(ev_wg[q]); }
        if (side) hipStreamDestroy(side);
        for (void* p : allocs) hipFree(p);
        for (void* p : {(void*)rec, (void*)perm, (void*)vbuf}) if (p) hipFree(p);
    }
    // packed kernels of conv layer l >= 1 in the forward / backward-data view
    Parts Wpf(int l) const { const size_t o = (size_t)(l - 1) * KC * NF; return Parts{{wpf[0] + o, wpf[1] + o, wpf[2] + o}}; }
    Parts Wpb(int l) const { const size_t o = (size_t)(l - 1) * KC * NF; return Parts{{wpb[0] + o, wpb[1] + o, nullptr}}; }
};
// conv layer l >= 1 in an AZRW-shaped vector (weights or gradients): kernel, then bn
inline float* layer_at(float* flat, int l) { return flat + OFF_BLOCK0 + (size_t)(l - 1) * LAYER; }
inline const float* layer_at(const float* flat, int l) { return flat + OFF_BLOCK0 + (size_t)(l - 1) * LAYER; }

TrainState* ctx_of(azr_engine* h) { return static_cast<TrainState*>(h->train); }

// a training call is entered: the handle's options, as they are now, are this call's
void opt_enter(azr_engine* h, TrainState* c)
{
    const azr_train_options& o = h->train_opt;
    c->opt = o;
    c->opt_default = o.lr == LR && o.l2 == L2_C && o.lr_schedule == AZR_LR_CONSTANT && o.warmup_steps == 0 && o.clip_norm == 0.0f && o.ema_decay == 0.0f;
}

// one hipMalloc per buffer, remembered by its owner (a TrainState's or a Slabs' allocs)
template <typename T>
int dalloc(azr_engine* h, std::vector<void*>& owner, T** p, size_t n)
{
    HIPCHK(h, hipMalloc((void**)p, n * sizeof(T)));
    owner.push_back(*p);
    return AZR_OK;
}

// grow-only buffers (rec, perm, vbuf): at least `need` elements behind the call; a failed allocation leaves none and capacity 0
int grow(azr_engine* h, void** p, size_t* cap, size_t need, size_t elem_size)
{
    if (need <= *cap) return AZR_OK;
    if (*p) hipFree(*p);
    *p = nullptr; *cap = 0;
    HIPCHK(h, hipMalloc(p, need * elem_size));
    *cap = need;
    return AZR_OK;
}

#define TRY(x)                 \
    do {                       \
        int rc__ = (x);        \
        if (rc__) return rc__; \
    } while (0)

// the weight gradient of one tower conv: 64 one-wave blocks (16 ci tiles x 4 co quarters) per slice of whole boards -> s.wpart[slice]
static void launch_wgrad(const Slabs& s, hipStream_t st, const Parts& apP, const Parts& dyP)
{
#ifdef AZR_TEST_HOOKS
    if (!s.plan.wg5) {
        hipLaunchKernelGGL(t_wgrad_rs, dim3(64 * s.wg_slices), dim3(64), Wg::LDS_BYTES, st, apP, dyP, s.wpart, s.M, s.wg_slices, s.wg_bps * NPOS);
        return;
    }
#endif
    hipLaunchKernelGGL(t_wgrad_g5<WG5_NC>, dim3(Wg5<WG5_NC>::BLOCKS_PER_SLICE * s.wg_parts), dim3(256), Wg5<WG5_NC>::LDS_BLOCK, st, apP, dyP, s.wpart, s.M / NPOS,
                       s.wg_slices, s.wg_bps);
}

// the handle's TrainState, created on the first call: installed only when it is complete (a failure on the way frees what was built)
int state_ensure(azr_engine* h)
{
    if (h->train) return AZR_OK;
    std::unique_ptr<TrainState> c(new TrainState());
    const int B = h->net.blocks;
    c->blocks = B; c->L = 2 * B + 1;
    c->count = net_param_count(B);
    auto alloc = [&](auto** p, size_t n) { return dalloc(h, c->allocs, p, n); };
    TRY(alloc(&c->g, c->count)); TRY(alloc(&c->m, c->count)); TRY(alloc(&c->v, c->count));
    TRY(alloc(&c->kind, c->count));
    TRY(alloc(&c->wpad, (size_t)KS * NF)); TRY(alloc(&c->gpad, (size_t)KS * NF));
    TRY(alloc(&c->mean, (size_t)c->L * NF)); TRY(alloc(&c->istd, (size_t)c->L * NF));
    TRY(alloc(&c->sums, (size_t)2 * NF));
    for (int q = 0; q < 3; q++) TRY(alloc(&c->wpf[q], (size_t)2 * B * KC * NF));
    for (int q = 0; q < 2; q++) TRY(alloc(&c->wpb[q], (size_t)2 * B * KC * NF));
    {
        int lo = 0, hi = 0;
        HIPCHK(h, hipDeviceGetStreamPriorityRange(&lo, &hi));   // (lo = the numerically greatest = least urgent)
        HIPCHK(h, hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, lo));
        for (int q = 0; q < 2; q++) {
            HIPCHK(h, hipEventCreateWithFlags(&c->ev_conv[q], hipEventDisableTiming));
            HIPCHK(h, hipEventCreateWithFlags(&c->ev_wg[q], hipEventDisableTiming));
        }
    }
    TRY(alloc(&c->hstat, (size_t)8)); TRY(alloc(&c->loss, (size_t)4));
    TRY(alloc(&c->cur, (size_t)CUR_N)); TRY(alloc(&c->lr, (size_t)1));
    TRY(alloc(&c->red, (size_t)2 * NG * NF)); TRY(alloc(&c->hsum, (size_t)8));
    TRY(alloc(&c->row, (size_t)1)); TRY(alloc(&c->sqpart, (size_t)SQ_BLOCKS));
    HIPCHK(h, hipMemset(c->row, 0, sizeof(StatRow)));
    HIPCHK(h, hipMemset(c->lr, 0, sizeof(float)));
    HIPCHK(h, hipMemset(c->cur, 0, CUR_N * sizeof(int)));
    for (float* z : {c->g, c->m, c->v}) HIPCHK(h, hipMemset(z, 0, c->count * 4));
    // parameter kinds: 1 = kernel (L2-regularised), 2 = BN gamma/beta and dense biases, 0 = BN moving statistics
    std::vector<uint8_t> kind(c->count, 0);
    auto fill = [&](size_t off, size_t n, uint8_t k) { std::fill(kind.begin() + off, kind.begin() + off + n, k); };
    fill(0, OFF_STEM_BN, 1);
    fill(OFF_STEM_BN, 14, 2);
    for (int l = 0; l < 2 * B; l++) {
        const size_t o = OFF_BLOCK0 + (size_t)l * LAYER;
        fill(o, (size_t)9 * NF * NF, 1);
        fill(o + (size_t)9 * NF * NF, 2 * NF, 2);
    }
    const size_t hh = OFF_BLOCK0 + (size_t)2 * B * LAYER;
    if (hh + HEAD_FLOATS != c->count) { h->err = "azr_nn_train: AZRW layout mismatch"; return AZR_E_STATE; }
    fill(hh + H_PI_W, 512, 1); fill(hh + H_PI_BN, 4, 2);
    fill(hh + H_PD_W, 3612, 1); fill(hh + H_PD_B, 43, 2);
    fill(hh + H_V_W, 256, 1); fill(hh + H_V_BN, 2, 2);
    fill(hh + H_V1_W, 10752, 1); fill(hh + H_V1_B, 256, 2);
    fill(hh + H_V2_W, 256, 1); fill(hh + H_V2_B, 1, 2);
    HIPCHK(h, hipMemcpy(c->kind, kind.data(), c->count, hipMemcpyHostToDevice));
    h->train = c.release();
    return AZR_OK;
}

// The state, and slabs for batches of BS records.  Another batch size frees the old slabs first (peak memory does not rise), builds the
// new ones into a local owner and installs them only when every allocation has succeeded: behind a failure the state has no slabs, and
// the next call builds them.  Nothing can see a batch size without its buffers.
int ctx_ensure(azr_engine* h, int BS)
{
    TRY(state_ensure(h));
    TrainState* c = ctx_of(h);
    if (c->slabs && c->slabs->BS == BS) return AZR_OK;
    // tuning switches, read when the slabs are (re)built — never in the step path
#ifdef AZR_TEST_HOOKS
    g_gemm_bf16x3 = !(hook_env("AZR_TRAIN_GEMM") && strcmp(hook_env("AZR_TRAIN_GEMM"), "f32") == 0);
    g_fuse_bwd = hook_env_int("AZR_TRAIN_FUSE", 1) != 0;
    g_fwd_f16 = !(hook_env("AZR_TRAIN_FWD") && strcmp(hook_env("AZR_TRAIN_FWD"), "bf16") == 0);
    g_fuse_apply = hook_env_int("AZR_TRAIN_FUSE_APPLY", 1) != 0;
    g_conv_q = hook_env_int("AZR_TRAIN_CONVQ", 1) != 0;
    g_wgrad_g5 = !(hook_env("AZR_TRAIN_WGRAD") && strcmp(hook_env("AZR_TRAIN_WGRAD"), "rs") == 0);
    HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(t_wgrad_rs), hipFuncAttributeMaxDynamicSharedMemorySize, Wg::LDS_BYTES));
#endif
    HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(t_wgrad_g5<WG5_NC>), hipFuncAttributeMaxDynamicSharedMemorySize, Wg5<WG5_NC>::LDS_BLOCK));
    c->slabs.reset();
    std::unique_ptr<Slabs> s(new Slabs());
    s->BS = BS; s->M = BS * NPOS;
    s->R = (s->M + RB - 1) / RB;
    // split-K of the weight-gradient GEMM (36 output tiles of 128 x 128): as many slices as keep <= 2 blocks per CU
    s->nz = std::max(1, std::min(512 / ((KC / GT) * (NF / GT)), (s->M + 1023) / 1024));
    s->kchunk = (((s->M + s->nz - 1) / s->nz) + K3 - 1) / K3 * K3;
    Plan& p = s->plan;
    p.sb = g_gemm_bf16x3 && s->M % K3 == 0;
    p.f16 = p.sb && g_fwd_f16;
    p.fap = p.f16 && g_fuse_bwd && g_fuse_apply;
    p.convq = p.fap && g_conv_q && BS <= 128;
    p.wg5 = g_wgrad_g5;
    p.fuse = p.sb && g_fuse_bwd;
    p.bap = p.fuse && g_fuse_apply;
    {
        // t_wgrad_g5: whole groups of 5 boards, as many slices as make the chip's 1024 SIMDs one block each
        using W = Wg5<WG5_NC>;
        const int want = 1024 / W::BLOCKS_PER_SLICE;
        int bps = std::max(W::GB, ((BS + want - 1) / want + W::GB - 1) / W::GB * W::GB);
#ifdef AZR_TEST_HOOKS
        // t_wgrad_rs: slices of 16 j boards (16 boards = 672 rows = 21 k-steps), about 256 blocks = 16 ci tiles x slices
        // (small batches — a rank's share of a data-parallel minibatch: 8-board slices, so that 64 records are 512 one-wave blocks)
        if (!p.wg5) bps = (BS <= 128 && BS % 8 == 0) ? 8 : 16 * std::max(1, BS / 256);
#endif
        s->wg_slices = (BS + bps - 1) / bps;
        s->wg_bps = bps;
        s->wg_parts = p.wg5 ? (s->wg_slices + 3) / 4 : s->wg_slices;
    }
    // (test hook AZR_TRAIN_FAIL_ALLOC=k, k >= 1 — libazr_hip_test.so only: the k-th allocation below fails before it reaches hipMalloc)
    const int fail = hook_env_int("AZR_TRAIN_FAIL_ALLOC", 0);
    auto alloc = [&](auto** p, size_t n) {
        if (fail > 0 && (size_t)fail == s->allocs.size() + 1) {
            h->err = "azr_nn_train: slab allocation " + std::to_string(fail) + " failed (injected by AZR_TRAIN_FAIL_ALLOC, no hipMalloc was called)";
            return (int)AZR_E_HIP;
        }
        return dalloc(h, s->allocs, p, n);
    };
    const size_t M = s->M, act = M * NF, L = c->L;
    TRY(alloc(&s->X0, M * SIN)); TRY(alloc(&s->col0, M * KS));
    TRY(alloc(&s->Y, act * L)); TRY(alloc(&s->A, act * L));
    TRY(alloc(&s->G, act)); TRY(alloc(&s->DS, act)); TRY(alloc(&s->DT, act)); TRY(alloc(&s->dY, act));
    TRY(alloc(&s->part, (size_t)s->R * 2 * NG * NF));
    TRY(alloc(&s->wpart, (size_t)std::max(s->nz, s->wg_slices) * KC * NF));
    // bf16 parts of the post-activations: the two leading parts are kept PER LAYER (the weight-gradient GEMM of the backward
    // pass wants exactly them: no second split), the third one only until the next forward conv has read it
    for (int q = 0; q < 3; q++) TRY(alloc(&s->ap[q], q < 2 ? act * L : act));
    for (int q = 0; q < 2; q++) { TRY(alloc(&s->dyp[q], act)); TRY(alloc(&s->dyp2[q], act)); }
    for (int q = 0; q < 2; q++) TRY(alloc(&s->af[q], act));
    TRY(alloc(&s->pv0, M * 4)); TRY(alloc(&s->dpv, M * 4));
    TRY(alloc(&s->fpi, (size_t)BS * 84)); TRY(alloc(&s->fv, (size_t)BS * 42)); TRY(alloc(&s->h1, (size_t)BS * 256));
    TRY(alloc(&s->vout, (size_t)BS)); TRY(alloc(&s->prob, (size_t)BS * 43)); TRY(alloc(&s->lossb, (size_t)BS * 2));
    TRY(alloc(&s->hpart, (size_t)BS * HP_FLOATS)); TRY(alloc(&s->cpart, (size_t)s->R * 3 * NF));
    TRY(alloc(&s->in88, (size_t)BS * 88)); TRY(alloc(&s->pit, (size_t)BS * 43)); TRY(alloc(&s->zt, (size_t)BS));
    HIPCHK(h, hipMemset(s->dpv, 0, M * 4 * sizeof(float)));
    c->slabs = std::move(s);
    return AZR_OK;
}

template <bool A_MCONTIG, bool B_KCONTIG, int BM = 128, int AMODE = 0, int BMODE = 0>
void gemm(hipStream_t st, const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K, int nz = 1,
          int kchunk = 0, size_t strideCz = 0)
{
    if (nz == 1) kchunk = K;
    hipLaunchKernelGGL((t_gemm<A_MCONTIG, B_KCONTIG, BM, AMODE, BMODE>), dim3((N + GT - 1) / GT, (M + BM - 1) / BM, nz), dim3(256), 0, st, A, lda, B, ldb,
                       C, ldc, M, N, K, kchunk, strideCz);
}

inline dim3 grid1(size_t n, int bs) { return dim3((unsigned)((n + bs - 1) / bs)); }

// RCCL, bound at run time: dlopen("librccl.so.1") returns the copy a host process has already loaded (PyTorch-ROCm ships one under
// the same soname) or /opt/rocm's — one RCCL, one HIP runtime per process, and libazr_hip.so itself carries no link dependency.
struct RcclApi {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    std::string err;
};
static void rccl_bind(RcclApi& api)
{
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        api.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
        if (api.lib) break;
    }
    if (!api.lib) { api.err = std::string("RCCL not found: ") + (dlerror() ? dlerror() : "dlopen failed"); return; }
    api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(dlsym(api.lib, "ncclGetUniqueId"));
    api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(dlsym(api.lib, "ncclCommInitRank"));
    api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(dlsym(api.lib, "ncclCommDestroy"));
    api.AllReduce = reinterpret_cast<decltype(api.AllReduce)>(dlsym(api.lib, "ncclAllReduce"));
    api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(dlsym(api.lib, "ncclGetErrorString"));
    if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.AllReduce || !api.GetErrorString) {
        api.err = "RCCL: a symbol is missing from the loaded library";
        api.lib = nullptr;
    }
}
RcclApi* rccl_api()   // bound once, whichever host thread asks first (the host CLI runs one thread per GPU)
{
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] { rccl_bind(api); });
    return &api;
}

// one all-reduce (sum, in place) of a device buffer over the ranks of a data-parallel step.  Native (azr_dp_init): ncclAllReduce on
// the engine's own stream — stream-ordered, the host never waits (86 of them per step at B = 20: with a host hand-over each they
// cost more than the step's kernels).  Otherwise through the caller's callback (a torch.distributed rehearsal over gloo, or any other
// transport): the engine's stream is drained first, the callback returns when the result is in place.
int dp_allreduce(azr_engine* h, const DpLink& k, void* dev, size_t count, int dtype)
{
    if (k.native) {
        RcclApi* R = rccl_api();
        const ncclResult_t rc = R->AllReduce(dev, dev, count, dtype ? ncclDouble : ncclFloat, ncclSum, static_cast<ncclComm_t>(h->dp_comm), h->stream);
        if (rc != ncclSuccess) { h->err = std::string("ncclAllReduce: ") + R->GetErrorString(rc); return AZR_E_HIP; }
        return AZR_OK;
    }
    if (!k.ar) return AZR_OK;
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const int rc = k.ar(k.ar_ctx, dev, count, dtype);
    if (rc) { h->err = "azr_nn_train_dp: the all-reduce callback failed with code " + std::to_string(rc); return AZR_E_STATE; }
    return AZR_OK;
}

// sums over the batch in a data-parallel step: [R local block partials of K rows -> one slab] -> all-reduce over the ranks; the finalize
// kernel then reads the slab as one block of partials
int reduce_parts(azr_engine* h, TrainState* c, int R, int K)
{
    hipLaunchKernelGGL(t_parts_sum, dim3(K), dim3(256), 0, h->stream, c->slabs->part, R, K, c->red);
    return dp_allreduce(h, c->link, c->red, (size_t)K * NF, 1);
}

// One tower conv of the split path: t_conv_q at small batches, else t_conv_rs (two parts), with the grid that goes with it.  Returns the
// number of blocks, i.e. of partials a statistics epilogue (FUSE != 0) leaves in bf.part.
template <int AMODE, int FUSE, bool F16, int PRO>
int launch_conv(const Slabs& s, hipStream_t st, const Parts& A, const Parts& W, float* out, const BwdFuse& bf, float oscale, const ProFuse& pf)
{
    const int BS = s.BS;
    if (s.plan.convq) {
        hipLaunchKernelGGL((t_conv_q<AMODE, FUSE, F16, PRO>), dim3(4 * BS), dim3(256), 0, st, A, W, out, BS, bf, oscale, pf);
        return BS;
    }
    hipLaunchKernelGGL((t_conv_rs<AMODE, 2, FUSE, F16, PRO>), dim3((BS + 1) / 2), dim3(256), 0, st, A, W, out, BS, bf, oscale, pf);
    return (BS + 1) / 2;
}

// The tower's forward pass on the minibatch already gathered into s.in88: planes -> stem -> conv layers 1 .. L - 1, leaving every
// layer's conv output (Yl) and post-activation (Al, with its bf16 parts) behind.
//   training:  batch statistics — taken in the conv's epilogue (FUSE = 2) or by t_bn_stats, all-reduced in a data-parallel step,
//              t_bn_finalize writes mean / 1/std and updates the moving averages; the stem kernel is padded every step (Adam moved it);
//   otherwise (the validation pass): c->mean / istd hold the MOVING statistics and c->wpad the padded stem kernel (azr_nn_validate,
//              once per call): no statistics kernels, no statistics epilogue (FUSE = 0), nothing but scratch is written.
int forward_tower(azr_engine* h, TrainState* c, bool training)
{
    hipStream_t st = h->stream;
    const Slabs& s = *c->slabs;
    const Plan& p = s.plan;
    const int M = s.M, R = s.R, L = c->L, world = c->link.world;
    const bool dp = c->link.dp();
    float* w = h->net.d_flat;
    const unsigned g4 = (unsigned)((s.act() / 4 + 255) / 256);
    uint16_t* const nil16 = nullptr;
    hipLaunchKernelGGL(t_planes, grid1((size_t)M * SIN, 256), dim3(256), 0, st, s.in88, M, s.X0);
    if (training) hipLaunchKernelGGL(t_stem_pad, grid1((size_t)KS * NF, 256), dim3(256), 0, st, w, c->wpad);
    hipLaunchKernelGGL((t_im2col<SIN>), grid1((size_t)M * 9, 4), dim3(256), 0, st, s.X0, s.col0, M);
    gemm<false, false, 64>(st, s.col0, KS, c->wpad, NF, s.Yl(0), NF, M, NF, KS);
    if (training) {
        hipLaunchKernelGGL((t_bn_stats<true>), dim3(R), dim3(1024), 0, st, s.Yl(0), M, s.part);
        if (dp) TRY(reduce_parts(h, c, R, 2 * NG));
        hipLaunchKernelGGL((t_bn_finalize<true>), dim3(NG), dim3(1024), 0, st, dp ? c->red : s.part, dp ? 1 : R,
                           (double)s.BS * world * 6 * NF, c->mean, c->istd, w + OFF_STEM_BN);
    }
    // (each layer's normalise kernel also writes the bf16 parts of its output and the fp16 pair: the next conv's A operand)
    hipLaunchKernelGGL((t_bn_apply<true>), dim3(g4), dim3(256), 0, st, s.Yl(0), c->mean, c->istd, w + OFF_STEM_BN, (const float*)nullptr, s.Al(0), M,
                       p.sb ? s.ap[0] : nil16, s.ap[1], p.f16 ? nil16 : s.ap[2], p.f16 ? s.af[0] : nil16, s.af[1]);
    const Parts none{{nullptr, nullptr, nullptr}}, af{{s.af[0], s.af[1], nullptr}};
    const BwdFuse bf{nullptr, nullptr, nullptr, nullptr, nullptr, training ? s.part : nullptr};
    for (int l = 1; l < L; l++) {
        float* bn = layer_at(w, l) + (size_t)9 * NF * NF;
        const float* S = (l % 2 == 0) ? s.Al(l - 2) : nullptr;  // second conv of a block adds the block input
        int parts = 0;   // block partials of the output's statistics that the conv's epilogue left (training)
        if (!p.sb) gemm<false, false, 64, 1, 0>(st, s.Al(l - 1), KC, layer_at(w, l), NF, s.Yl(l), NF, M, NF, KC);
        else if (p.fap && l >= 2) {
            // Fused mode (fp16 forward + epilogue statistics + staging-path normalise): layer l - 1's normalise step is not a kernel of
            // its own — this conv computes A_m = relu(BN(Y_m) (+ S)), m = l - 1, while it stages its operand and writes A_m and its bf16
            // parts out; only the stem (row-wise BN) and the last layer (the heads read it) keep t_bn_apply.
            const int m = l - 1;
            const ProFuse pf{s.Yl(m), (m % 2 == 0) ? (const float*)s.Al(m - 2) : (const float*)nullptr, nullptr, c->mean + m * NF, c->istd + m * NF,
                             layer_at(w, m) + (size_t)9 * NF * NF, nullptr, 0.0f, s.Al(m), const_cast<uint16_t*>(s.Ap(m).p[0]),
                             const_cast<uint16_t*>(s.Ap(m).p[1])};
            if (training) parts = launch_conv<1, 2, true, 1>(s, st, none, c->Wpf(l), s.Yl(l), bf, 1.0f / FWD_WSCALE, pf);
            else launch_conv<1, 0, true, 1>(s, st, none, c->Wpf(l), s.Yl(l), bf, 1.0f / FWD_WSCALE, pf);
        } else if (p.f16) {   // operand = the fp16 pair the previous normalise kernel wrote (layer 1: the stem's)
            if (training && p.fuse) parts = launch_conv<1, 2, true, 0>(s, st, af, c->Wpf(l), s.Yl(l), bf, 1.0f / FWD_WSCALE, ProFuse{});
            else launch_conv<1, 0, true, 0>(s, st, af, c->Wpf(l), s.Yl(l), bf, 1.0f / FWD_WSCALE, ProFuse{});   // (training: AZR_TRAIN_FUSE=0)
        }
#ifdef AZR_TEST_HOOKS   // AZR_TRAIN_FWD=bf16, the older formulation of the same conv: three bf16 parts, 6 passes (libazr_hip_test.so only)
        else hipLaunchKernelGGL((t_conv_rs<1, 3>), dim3((s.BS + 1) / 2), dim3(256), 0, st, s.Ap(l - 1), c->Wpf(l), s.Yl(l), s.BS, BwdFuse{}, 1.0f, ProFuse{});
#endif
        if (training) {
            const int Rf = parts ? parts : R;
            if (!parts) hipLaunchKernelGGL((t_bn_stats<false>), dim3(R), dim3(1024), 0, st, s.Yl(l), M, s.part);
            if (dp) TRY(reduce_parts(h, c, Rf, 2));
            hipLaunchKernelGGL((t_bn_finalize<false>), dim3(8), dim3(1024), 0, st, dp ? c->red : s.part, dp ? 1 : Rf, (double)M * world,
                               c->mean + l * NF, c->istd + l * NF, bn);
        }
        if (p.fap && l + 1 < L) continue;   // the next conv normalises this layer's output itself
        hipLaunchKernelGGL((t_bn_apply<false>), dim3(g4), dim3(256), 0, st, s.Yl(l), c->mean + l * NF, c->istd + l * NF, bn, S, s.Al(l), M,
                           (p.sb && l + 1 < L) ? const_cast<uint16_t*>(s.Ap(l).p[0]) : nil16, const_cast<uint16_t*>(s.Ap(l).p[1]),
                           p.f16 ? nil16 : s.ap[2], (p.f16 && l + 1 < L) ? s.af[0] : nil16, s.af[1]);
    }
    return AZR_OK;
}

// what the backward loop carries from layer l to layer l - 1
struct LayerCarry {
    int fused_parts = 0;            // t_conv_rs<2, 2, 1>, the backward-data conv of layer l, has left stage 1 of layer l - 1's batch-norm backward
                                    // behind: its block partials are already in s.part, this many blocks of them
    float* pending_sum = nullptr;   // the slice sum of the layer above is launched together with this layer's BN-backward stage 2 (t_sum_slices_fin)
    int side_used = 0;              // the layer parities whose weight gradient ran on the side stream
};

// One optimiser step on the minibatch already gathered into s.in88 / pit / zt: what every stage reads, and the stages in the order
// run() calls them.  (Data-parallel: BS / M are this rank's shard, BSg / Mg the whole minibatch every statistic and mean refers to.)
struct Step {
    azr_engine* const h;
    TrainState* const c;
    const Slabs& s = *c->slabs;
    const Plan& p = s.plan;
    const hipStream_t st = h->stream;
    const int M = s.M, R = s.R, BS = s.BS, BSg = BS * c->link.world, Mg = M * c->link.world;
    const bool dp = c->link.dp();
    const float gscale = 1.0f / (float)c->link.world, invM = 1.0f / (float)Mg;
    float* const w = h->net.d_flat;
    float* const g = c->g;
    const size_t wn = (size_t)KC * NF, hh = OFF_BLOCK0 + (size_t)2 * c->blocks * LAYER;
    float* const hp = w + hh;   // the heads' part of w
    float* const gh = g + hh;   // ... and of g
    const unsigned g4 = (unsigned)((s.act() / 4 + 255) / 256);
    uint16_t* const nil16 = nullptr;

    int heads_forward(float* d_acc) const
    {
        const float* H = s.Al(c->L - 1);
        hipLaunchKernelGGL(t_head_conv, grid1((size_t)M, 4), dim3(256), 0, st, H, hp, s.pv0, M);
        hipLaunchKernelGGL(t_head_bn_sums, dim3(1), dim3(1024), 0, st, s.pv0, M, c->hsum);
        if (dp) TRY(dp_allreduce(h, c->link, c->hsum, 6, 1));
        hipLaunchKernelGGL(t_head_bn_stats, dim3(1), dim3(64), 0, st, (const double*)c->hsum, (double)Mg, hp, c->hstat);
        hipLaunchKernelGGL(t_head_fwd, dim3(BS), dim3(256), 0, st, s.pv0, hp, c->hstat, s.pit, s.zt, s.fpi, s.fv, s.h1, s.vout, s.prob, s.lossb);
        hipLaunchKernelGGL(t_loss, dim3(1), dim3(1), 0, st, s.lossb, BS, BSg, c->loss);
        if (dp) TRY(dp_allreduce(h, c->link, c->loss, 2, 0));
        hipLaunchKernelGGL(t_loss_acc, dim3(1), dim3(1), 0, st, (const float*)c->loss, d_acc);
        return AZR_OK;
    }

    int heads_backward() const
    {
        const float* H = s.Al(c->L - 1);
        hipLaunchKernelGGL(t_head_bwd, dim3(BS), dim3(256), 0, st, hp, s.pit, s.zt, s.fpi, s.fv, s.h1, s.vout, s.prob, BSg, s.dpv, s.hpart);
        hipLaunchKernelGGL(t_head_reduce, grid1(HP_FLOATS, 256), dim3(256), 0, st, s.hpart, BS, gh);
        hipLaunchKernelGGL(t_head_bn_bwd_sums, dim3(1), dim3(1024), 0, st, s.pv0, c->hstat, M, (const float*)s.dpv, c->hsum);
        if (dp) TRY(dp_allreduce(h, c->link, c->hsum, 6, 1));
        hipLaunchKernelGGL(t_head_bn_bwd, dim3((M + 1023) / 1024), dim3(1024), 0, st, s.pv0, hp, c->hstat, M, (const double*)c->hsum, (float)Mg, gscale, s.dpv, gh);
        hipLaunchKernelGGL(t_head_conv_bwd, dim3(R), dim3(256), 0, st, H, s.dpv, hp, M, s.G, s.cpart);
        hipLaunchKernelGGL(t_head_conv_bwd_finalize, dim3(1), dim3(256), 0, st, s.cpart, R, gh);
        return AZR_OK;
    }

    // gradient w.r.t. layer l's post-activation output: G for the second conv of a block, DT for the first; the conv's input gradient
    // goes to the other one
    static bool second(int l) { return l % 2 == 0; }
    const float* dOut(int l) const { return second(l) ? s.G : s.DT; }
    float* dIn(int l) const { return second(l) ? s.DT : s.G; }

    // both forms of a layer's backward pass begin with the sums of its batch-norm backward: stage 1 (unless the conv of the layer above
    // left it), the ranks' sum, stage 2 — with the slice sum that is still pending, in one launch where that is possible
    int layer_bn_sums(int l, LayerCarry& k) const
    {
        float* gbn = layer_at(g, l) + wn;
        const int Rl = k.fused_parts ? k.fused_parts : R;
        if (!k.fused_parts)
            hipLaunchKernelGGL((t_bn_bwd_stats<false>), dim3(R), dim3(1024), 0, st, dOut(l), s.Al(l), s.Yl(l), c->mean + l * NF, c->istd + l * NF, M, s.part);
        if (dp) TRY(reduce_parts(h, c, Rl, 2));
        if (k.pending_sum && !dp && k.fused_parts) {
            hipLaunchKernelGGL(t_sum_slices_fin, dim3(8 + (unsigned)((wn + 1023) / 1024)), dim3(1024), 0, st, s.wpart, s.wg_parts, wn, k.pending_sum, s.part,
                               Rl, gbn, c->sums, gscale);
        } else {
            if (k.pending_sum) hipLaunchKernelGGL(t_sum_slices, grid1(wn, 256), dim3(256), 0, st, s.wpart, s.wg_parts, wn, k.pending_sum);
            hipLaunchKernelGGL((t_bn_bwd_finalize<false>), dim3(8), dim3(1024), 0, st, dp ? c->red : s.part, dp ? 1 : Rl, gbn, c->sums, gscale);
        }
        k.pending_sum = nullptr;
        return AZR_OK;
    }

    // The product's form (plan.bap).  dY is computed in the backward-data conv's staging path (t_bn_bwd_apply's arithmetic; its two bf16
    // parts and, where the layer closes a block, dz = the shortcut gradient DS are written out on the way), so that conv runs FIRST and
    // the weight-gradient GEMM reads the parts it left behind — on the side stream (TrainState::side), from the set of its layer parity
    int layer_bwd_fused(int l, LayerCarry& k) const
    {
        const int L = c->L;
        const Parts apP{{s.Ap(l - 1).p[0], s.Ap(l - 1).p[1], nullptr}};
        const bool beside = p.convq && !c->link.native;   // (in-stream RCCL collectives and cross-stream edges do not mix: 16 ms per step measured)
        const int q = beside ? (l & 1) : 0;
        uint16_t* const* dq = q ? s.dyp2 : s.dyp;
        const Parts dyP{{dq[0], dq[1], nullptr}};
        if (beside && l + 2 <= L - 1) HIPCHK(h, hipStreamWaitEvent(st, c->ev_wg[q], 0));   // layer l + 2's weight gradient has read this set
        const ProFuse pf{dOut(l), s.Al(l), s.Yl(l), c->mean + l * NF, c->istd + l * NF, layer_at(w, l) + wn, c->sums, invM, second(l) ? s.DS : (float*)nullptr,
                         dq[0], dq[1]};
        const Parts none{{nullptr, nullptr, nullptr}};
        k.fused_parts = 0;
        if (l >= 2) {
            const BwdFuse bf{second(l) ? (const float*)nullptr : (const float*)s.DS, s.Al(l - 1), s.Yl(l - 1), c->mean + (l - 1) * NF, c->istd + (l - 1) * NF, s.part};
            k.fused_parts = launch_conv<2, 1, false, 2>(s, st, none, c->Wpb(l), dIn(l), bf, 1.0f, pf);
        } else {
            launch_conv<2, 0, false, 2>(s, st, none, c->Wpb(l), dIn(l), BwdFuse{}, 1.0f, pf);
            if (!second(l)) hipLaunchKernelGGL(t_add, dim3(g4), dim3(256), 0, st, dIn(l), s.DS, s.act() / 4);
        }
        if (!beside) {  // large batches: the chain's kernels and the weight gradient each fill the register files on their own (368 and 280
                        // VGPRs: no SIMD holds a wave of both) and nothing overlaps: one stream.  (Measured at batch 512: the branch on the
                        // side stream 11.16 ms per step, only its slice sums there 11.28, one stream 11.1 — a cross-stream edge costs the
                        // chain a barrier packet per layer, about what hiding the 10-us slice sum saves.)
            launch_wgrad(s, st, apP, dyP);
            k.pending_sum = layer_at(g, l);   // summed by the next layer's launch (t_sum_slices_fin), or behind the loop
            return AZR_OK;
        }
        // small batches (a rank's share of a data-parallel minibatch): the chain's kernels leave most of the chip idle, the branch runs beside them
        HIPCHK(h, hipEventRecord(c->ev_conv[q], st));
        HIPCHK(h, hipStreamWaitEvent(c->side, c->ev_conv[q], 0));
        launch_wgrad(s, c->side, apP, dyP);
        hipLaunchKernelGGL(t_sum_slices, grid1(wn, 256), dim3(256), 0, c->side, s.wpart, s.wg_parts, wn, layer_at(g, l));
        HIPCHK(h, hipEventRecord(c->ev_wg[q], c->side));
        k.side_used |= 1 << q;
        return AZR_OK;
    }

    // The unfused form: normalise kernel, weight gradient, backward-data conv.  In the product library it is reached only by batches whose
    // row count is no multiple of the 32-deep k-tile: the fp32-MFMA GEMMs.  The split-bf16 kernels WITHOUT the staging-path fusions are
    // older formulations, compiled into libazr_hip_test.so only.
    int layer_bwd_unfused(int l, LayerCarry& k) const
    {
        const bool sb = p.sb;
        const Parts apP{{s.Ap(l - 1).p[0], s.Ap(l - 1).p[1], nullptr}}, dyP{{s.dyp[0], s.dyp[1], nullptr}};
        // (the split-bf16 kernels read the two parts of dY; its fp32 image is only written for the fp32-MFMA GEMMs)
        hipLaunchKernelGGL((t_bn_bwd_apply<false>), dim3(g4), dim3(256), 0, st, dOut(l), s.Al(l), s.Yl(l), c->mean + l * NF, c->istd + l * NF, layer_at(w, l) + wn,
                           c->sums, invM, sb ? (float*)nullptr : s.dY, second(l) ? s.DS : (float*)nullptr, M, sb ? s.dyp[0] : nil16, s.dyp[1]);
        // dW = col(input)^T x dY  (implicit im2col, split-K over the M rows)
#ifdef AZR_TEST_HOOKS
        if (sb) {
            launch_wgrad(s, st, apP, dyP);
        } else
#endif
        gemm<true, false, 128, 1, 0>(st, s.Al(l - 1), KC, s.dY, NF, s.wpart, NF, KC, NF, M, s.nz, s.kchunk, wn);
        hipLaunchKernelGGL(t_sum_slices, grid1(wn, 256), dim3(256), 0, st, s.wpart, sb ? s.wg_parts : s.nz, wn, layer_at(g, l));
        // d(input) = transposed conv of dY with W: the same implicit GEMM with negated taps and W read as [tap][co] x [ci]
        k.fused_parts = 0;
#ifdef AZR_TEST_HOOKS
        if (p.fuse && l >= 2) {   // + the shortcut gradient (first conv of a block), + stage 1 of layer l - 1's BN backward
            k.fused_parts = (BS + 1) / 2;
            hipLaunchKernelGGL((t_conv_rs<2, 2, 1>), dim3(k.fused_parts), dim3(256), 0, st, dyP, c->Wpb(l), dIn(l), BS,
                               BwdFuse{second(l) ? (const float*)nullptr : (const float*)s.DS, s.Al(l - 1), s.Yl(l - 1), c->mean + (l - 1) * NF,
                                       c->istd + (l - 1) * NF, s.part}, 1.0f, ProFuse{});
            return AZR_OK;
        }
        if (sb) hipLaunchKernelGGL((t_conv_rs<2, 2>), dim3((BS + 1) / 2), dim3(256), 0, st, dyP, c->Wpb(l), dIn(l), BS, BwdFuse{}, 1.0f, ProFuse{});
        else
#endif
        gemm<false, true, 64, 2, 3>(st, s.dY, KC, layer_at(w, l), NF, dIn(l), NF, M, NF, KC);
        if (!second(l)) hipLaunchKernelGGL(t_add, dim3(g4), dim3(256), 0, st, dIn(l), s.DS, s.act() / 4);  // + shortcut gradient
        return AZR_OK;
    }

    // stem: parameters only
    int stem_backward() const
    {
        hipLaunchKernelGGL((t_bn_bwd_stats<true>), dim3(R), dim3(1024), 0, st, s.G, s.Al(0), s.Yl(0), c->mean, c->istd, M, s.part);
        if (dp) TRY(reduce_parts(h, c, R, 2 * NG));
        hipLaunchKernelGGL((t_bn_bwd_finalize<true>), dim3(NG), dim3(1024), 0, st, dp ? c->red : s.part, dp ? 1 : R, g + OFF_STEM_BN, c->sums, gscale);
        hipLaunchKernelGGL((t_bn_bwd_apply<true>), dim3(g4), dim3(256), 0, st, s.G, s.Al(0), s.Yl(0), c->mean, c->istd, w + OFF_STEM_BN, c->sums,
                           1.0f / ((float)BSg * 6 * NF), s.dY, (float*)nullptr, M, nil16, nil16);
        gemm<true, false>(st, s.col0, KS, s.dY, NF, s.wpart, NF, KS, NF, M, s.nz, s.kchunk, (size_t)KS * NF);
        hipLaunchKernelGGL(t_sum_slices, grid1((size_t)KS * NF, 256), dim3(256), 0, st, s.wpart, s.nz, (size_t)KS * NF, c->gpad);
        hipLaunchKernelGGL(t_stem_unpad, grid1((size_t)9 * 13 * NF, 256), dim3(256), 0, st, c->gpad, g);
        return AZR_OK;
    }

    // Adam: with every option at its default, the reference's step; else [norm ->] schedule -> Adam on the clipped gradient (+ EMA),
    // behind the all-reduce so that every rank computes the same norm
    int update() const
    {
        c->last_default = c->opt_default;
        if (c->opt_default) {
            hipLaunchKernelGGL(t_tick_lr, dim3(1), dim3(1), 0, st, c->cur, c->lr);
            hipLaunchKernelGGL(t_adam, grid1(c->count, 256), dim3(256), 0, st, w, g, c->m, c->v, c->kind, c->count, (const float*)c->lr);
            return AZR_OK;
        }
        const azr_train_options& o = c->opt;
        const float l2x2 = 2.0f * o.l2;
        if (o.clip_norm > 0.0f) {
            hipLaunchKernelGGL(t_grad_sqsum, dim3(SQ_BLOCKS), dim3(256), 0, st, (const float*)w, (const float*)g, (const uint8_t*)c->kind, c->count, l2x2, c->sqpart);
            hipLaunchKernelGGL(t_grad_sqsum_final, dim3(1), dim3(256), 0, st, (const double*)c->sqpart, (double)o.clip_norm, c->row);
        }
        const Sched sc = {(double)o.lr, (double)o.lr_min / (double)o.lr, (double)o.decay_gamma, o.lr_schedule, o.warmup_steps, o.total_steps,
                          o.decay_period, o.clip_norm > 0.0f ? 1 : 0};
        hipLaunchKernelGGL(t_tick_lr_sched, dim3(1), dim3(1), 0, st, c->cur, c->lr, c->row, sc);
        if (o.ema_decay > 0.0f) {
            hipLaunchKernelGGL(t_adam_opt<true>, grid1(c->count, 256), dim3(256), 0, st, w, (const float*)g, c->m, c->v, c->e, (const uint8_t*)c->kind, c->count,
                               (const float*)c->lr, (const StatRow*)c->row, l2x2, o.ema_decay);
            c->ema_steps++;
        } else {
            hipLaunchKernelGGL(t_adam_opt<false>, grid1(c->count, 256), dim3(256), 0, st, w, (const float*)g, c->m, c->v, (float*)nullptr, (const uint8_t*)c->kind,
                               c->count, (const float*)c->lr, (const StatRow*)c->row, l2x2, 0.0f);
        }
        return AZR_OK;
    }

    int run(float* d_acc) const
    {
        if (p.sb) {
            const dim3 pg((unsigned)((wn / 8 + 255) / 256), 2 * c->blocks);
            hipLaunchKernelGGL((t_pack_w<3>), pg, dim3(256), 0, st, w, 0, c->wpf[0], c->wpf[1], c->wpf[2], p.f16 ? FWD_WSCALE : 0.0f, c->cur + CUR_RANGE);
            hipLaunchKernelGGL((t_pack_w<2>), pg, dim3(256), 0, st, w, 1, c->wpb[0], c->wpb[1], (uint16_t*)nullptr);
        }
        TRY(forward_tower(h, c, true));
        TRY(heads_forward(d_acc));
        TRY(heads_backward());
        LayerCarry k;
        for (int l = c->L - 1; l >= 1; l--) {
            TRY(layer_bn_sums(l, k));
            TRY(p.bap ? layer_bwd_fused(l, k) : layer_bwd_unfused(l, k));
        }
        if (k.pending_sum) hipLaunchKernelGGL(t_sum_slices, grid1(wn, 256), dim3(256), 0, st, s.wpart, s.wg_parts, wn, k.pending_sum);
        // the weight-gradient branch joins: the stem below reuses its split-K buffer, and the gradient vector is complete behind it
        for (int q = 0; q < 2; q++) if ((k.side_used >> q) & 1) HIPCHK(h, hipStreamWaitEvent(st, c->ev_wg[q], 0));
        TRY(stem_backward());
        // data-parallel: the ranks' gradient vectors add up to the gradient of the whole minibatch (one RCCL all-reduce of count floats:
        // 94.7 MB at B = 20); every rank then takes the same Adam step
        if (dp) TRY(dp_allreduce(h, c->link, g, c->count, 0));
        TRY(update());
        hipLaunchKernelGGL(t_tick_batch, dim3(1), dim3(1), 0, st, c->cur, BSg);
        HIPCHK(h, hipGetLastError());
        return AZR_OK;
    }
};

// One minibatch step = gather + forward + backward + Adam.  Everything that changes from step to step (minibatch offset, Adam step
// count, learning rate) lives in device memory; the launches are plain stream launches (replaying the step as a captured hipGraph
// measured the same: the ~3 us between consecutive kernels is device-side, not host launch cost).
int run_step(azr_engine* h, TrainState* c)
{
    const Slabs& s = *c->slabs;
    c->step++;
    if (c->opt.ema_decay > 0.0f && !c->e) {   // the EMA vector starts as the weights from before its first step
        TRY(dalloc(h, c->allocs, &c->e, c->count));
        HIPCHK(h, hipMemcpyAsync(c->e, h->net.d_flat, c->count * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        c->ema_steps = 0;
    }
    hipLaunchKernelGGL(t_gather, dim3(s.BS), dim3(64), 0, h->stream, c->rec, c->perm, (const int*)c->cur, s.BS, s.in88, s.pit, s.zt);
    return Step{h, c}.run(c->loss + 2);
}

// The validation pass (inference mode) on the minibatch already gathered into s.in88 / pit / zt: the forward kernels of the step at the
// step's precision (forward_tower with c->mean / istd / hstat holding the MOVING statistics: t_bn_moving, once per call), then the
// fused heads (t_head_eval) write the per-record losses to lossb.  Reads the weights, writes only scratch.
int eval_step(azr_engine* h, TrainState* c, float* lossb)
{
    const Slabs& s = *c->slabs;
    TRY(forward_tower(h, c, false));
    const float* hp = h->net.d_flat + OFF_BLOCK0 + (size_t)2 * c->blocks * LAYER;
    hipLaunchKernelGGL(t_head_eval, dim3(s.BS), dim3(256), 0, h->stream, (const float*)s.Al(c->L - 1), hp, (const float*)c->hstat, (const float*)s.pit,
                       (const float*)s.zt, lossb);
    return AZR_OK;
}

// Behind an epoch (or a single step): did a conv weight leave the range of the fp16-pair forward conv (t_pack_w's flag: |w| >= 64, or
// not a number), or did the losses stop being numbers?  Then the device copy of the weights and the optimiser state are poisoned: the
// call fails loudly, the weights the handle had before the call (its host AZRW copy) are put back and the optimiser state is dropped.
int step_health(azr_engine* h, TrainState* c, float loss_pi, float loss_v)
{
    int flag = 0;
    HIPCHK(h, hipMemcpyAsync(&flag, c->cur + CUR_RANGE, sizeof flag, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (!flag && std::isfinite(loss_pi) && std::isfinite(loss_v)) return AZR_OK;
    HIPCHK(h, hipMemcpyAsync(h->net.d_flat, h->flat.data(), h->flat.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    azr::train_free(h);
    h->err = flag ? "azr_nn_train: a conv weight left the range of the fp16-pair forward conv (|w| must stay below 64) or is not a number; "
                    "the weights from before the call have been restored and the optimiser state dropped"
                  : "azr_nn_train: the loss is not a number (diverged step); the weights from before the call have been restored and the "
                    "optimiser state dropped";
    return AZR_E_INVALID_ARGUMENT;
}

// after training: device master copy -> host AZRW copy -> refold / repack for inference
int finish(azr_engine* h)
{
    HIPCHK(h, hipMemcpyAsync(h->flat.data(), h->net.d_flat, h->flat.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return net_upload(h);
}

int upload_records(azr_engine* h, TrainState* c, const void* rec, size_t n)
{
    TRY(grow(h, (void**)&c->rec, &c->rec_cap, n, 265));
    TRY(grow(h, (void**)&c->perm, &c->perm_cap, n, sizeof(int)));
    HIPCHK(h, hipMemcpyAsync(c->rec, rec, n * 265, hipMemcpyHostToDevice, h->stream));
    return AZR_OK;
}

// the call's cursor: the first minibatch, the state's step count, this rank's offset inside a minibatch, a cleared range flag
int upload_cursor(azr_engine* h, TrainState* c, int rank_offset)
{
    int cur[CUR_N] = {};
    cur[CUR_STEP] = (int)c->step;
    cur[CUR_RANK] = rank_offset;
    HIPCHK(h, hipMemcpyAsync(c->cur, cur, sizeof cur, hipMemcpyHostToDevice, h->stream));
    return AZR_OK;
}

// The validation pass's buffer vbuf, in floats: this header | batch means [nb][2] | per-record terms [nb * BS][2]
struct ValHdr {
    float sum[2];   // t_val_sum: the batch means' sums (policy, value)
    int range;      // t_pack_w's range flag
    int pad;
    int cur[CUR_N];   // t_gather's view of cur: {offset in perm, -, 0, -}
};
static_assert(sizeof(ValHdr) == 32 && offsetof(ValHdr, cur) == 16, "the validation buffer's header");
constexpr size_t val_mean(size_t k) { return sizeof(ValHdr) / sizeof(float) + 2 * k; }             // batch k's two means
constexpr size_t val_rec(size_t nb, size_t i) { return val_mean(nb) + 2 * i; }                     // record i's two terms

}  // namespace

namespace azr {
void train_free(azr_engine* h)
{
    delete ctx_of(h);
    h->train = nullptr;
}
}  // namespace azr

#define ENTER(h)                                 \
    if (!(h)) return AZR_E_BAD_HANDLE;           \
    HIPCHK(h, hipSetDevice((h)->cfg.device))

extern "C" int azr_nn_train_batch(azr_engine* h, const void* rec265_host, int n, float* loss_pi, float* loss_v)
{
    ENTER(h);
    if (!h->weights_set) { h->err = "azr_nn_train_batch: no weights"; return AZR_E_STATE; }
    if (!rec265_host || n < 2) { h->err = "azr_nn_train_batch: need a minibatch of at least 2 records"; return AZR_E_INVALID_ARGUMENT; }
    TRY(ctx_ensure(h, n));
    TrainState* c = ctx_of(h);
    c->link = DpLink{};
    opt_enter(h, c);
    TRY(upload_records(h, c, rec265_host, (size_t)n));
    std::vector<int> id(n);
    for (int i = 0; i < n; i++) id[i] = i;
    HIPCHK(h, hipMemcpyAsync(c->perm, id.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->stream));
    TRY(upload_cursor(h, c, 0));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemsetAsync(c->loss + 2, 0, 2 * sizeof(float), h->stream));
    TRY(run_step(h, c));
    float l[2];
    HIPCHK(h, hipMemcpyAsync(l, c->loss, sizeof l, hipMemcpyDeviceToHost, h->stream));
    TRY(step_health(h, c, l[0], l[1]));
    TRY(finish(h));
    if (loss_pi) *loss_pi = l[0];
    if (loss_v) *loss_v = l[1];
    return AZR_OK;
}

// AlphaZeroNN::train for rank `rank` of `world` data-parallel ranks (world = 1: the reference's single-GPU training).  Every
// rank holds ALL n records and the same shuffle stream; of each minibatch of batch_size records rank r takes the slice
// [r * batch_size / world, (r + 1) * batch_size / world).
static int train_impl(azr_engine* h, const void* rec265_host, size_t n, int epochs, int batch_size, uint32_t* shuffle_rng_state, int rank,
                      int world, azr_allreduce_fn ar, void* ar_ctx, float* loss_pi_host, float* loss_v_host, bool dp_call = false)
{
    if (!h->weights_set) { h->err = "azr_nn_train: no weights"; return AZR_E_STATE; }
    if (!rec265_host || epochs < 0 || batch_size < 2) { h->err = "azr_nn_train: bad arguments"; return AZR_E_INVALID_ARGUMENT; }
    // no callback: the handle's own communicator (azr_dp_init) carries the sums.  (Test hook AZR_DP_LOOPBACK=1 — libazr_hip_test.so only, a
    // timing aid of tools/train_bench.py: a ONE-rank communicator stands in for `world` ranks — rank 0's share of the step with every
    // collective in the stream, sums stay local, so the weights it leaves are NOT those of a real step.  The product library has no such
    // switch: a communicator of another world size is refused.)
    const bool loopback = hook_env_int("AZR_DP_LOOPBACK", 0) != 0;
    const bool native = dp_call && !ar && h->dp_comm && ((h->dp_world == world && h->dp_rank == rank) || (loopback && h->dp_world == 1 && rank == 0));
    if (world < 1 || rank < 0 || rank >= world || (world > 1 && !ar && !native) || batch_size % world != 0 || batch_size / world < 2) {
        h->err = "azr_nn_train_dp: need 0 <= rank < world, batch_size a multiple of world with >= 2 records per rank, and either an all-reduce "
                 "callback or a communicator of exactly this rank / world (azr_dp_init)";
        return AZR_E_INVALID_ARGUMENT;
    }
    const int local_bs = batch_size / world;
    const size_t batches = n / (size_t)batch_size;  // the remainder of an epoch is dropped (alphazero_nn.cpp:374)
    std::minstd_rand0 eng;                          // RNG.getEngine() (src/rng.h:5-50): the caller's stream continues here
    if (shuffle_rng_state) {
        // a raw engine state, as azr_engine_set_rng takes it; 0 is not a state of minstd_rand0
        if (*shuffle_rng_state == 0 || *shuffle_rng_state >= 2147483647u) { h->err = "azr_nn_train: bad engine state"; return AZR_E_INVALID_ARGUMENT; }
        eng.seed(*shuffle_rng_state);
    }
    std::vector<int> order(n);
    for (size_t i = 0; i < n; i++) order[i] = (int)i;
    TrainState* c = nullptr;
    if (batches > 0 && epochs > 0) {
        TRY(ctx_ensure(h, local_bs));
        c = ctx_of(h);
        c->link = DpLink{world, rank, ar, ar_ctx, native};
        opt_enter(h, c);
        TRY(upload_records(h, c, rec265_host, n));
    }
    int rc = AZR_OK;
    for (int e = 0; e < epochs && rc == AZR_OK; e++) {
        std::shuffle(order.begin(), order.end(), eng);  // alphazero_nn.cpp:372 (same libstdc++ algorithm, same engine)
        float l[2] = {NAN, NAN};
        if (batches > 0) {
            HIPCHK(h, hipMemcpyAsync(c->perm, order.data(), n * sizeof(int), hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipMemsetAsync(c->loss + 2, 0, 2 * sizeof(float), h->stream));
            TRY(upload_cursor(h, c, rank * local_bs));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            for (size_t b = 0; b < batches && rc == AZR_OK; b++) rc = run_step(h, c);
            if (rc) break;
            HIPCHK(h, hipMemcpyAsync(l, c->loss + 2, sizeof l, hipMemcpyDeviceToHost, h->stream));
            rc = step_health(h, c, l[0], l[1]);   // (synchronises the stream)
            if (rc) { c = nullptr; break; }       // (the state is gone with the poisoned optimiser state)
            l[0] /= (float)batches;
            l[1] /= (float)batches;
        }
        if (loss_pi_host) loss_pi_host[e] = l[0];
        if (loss_v_host) loss_v_host[e] = l[1];
    }
    if (c) c->link = DpLink{};
    if (rc) return rc;
    if (shuffle_rng_state) {
        // minstd_rand0 has no state accessor; operator<< prints the state as decimal text
        std::ostringstream os;
        os << eng;
        *shuffle_rng_state = (uint32_t)std::stoul(os.str());
    }
    if (batches > 0 && epochs > 0) TRY(finish(h));
    return AZR_OK;
}

extern "C" int azr_nn_train(azr_engine* h, const void* rec265_host, size_t n, int epochs, int batch_size, uint32_t* shuffle_rng_state,
                            float* loss_pi_host, float* loss_v_host)
{
    ENTER(h);
    return train_impl(h, rec265_host, n, epochs, batch_size, shuffle_rng_state, 0, 1, nullptr, nullptr, loss_pi_host, loss_v_host);
}

extern "C" int azr_nn_train_dp(azr_engine* h, const void* rec265_host, size_t n, int epochs, int batch_size, uint32_t* shuffle_rng_state,
                               int rank, int world, azr_allreduce_fn allreduce, void* ctx, float* loss_pi_host, float* loss_v_host)
{
    ENTER(h);
    return train_impl(h, rec265_host, n, epochs, batch_size, shuffle_rng_state, rank, world, allreduce, ctx, loss_pi_host, loss_v_host, true);
}

// The validation phase of AlphaZeroNN::trainCrossValidation (alphazero_nn.cpp:512-548): every batch of the call is queued back to back
// (gather with the device-side offset ValHdr::cur, eval_step), then the batch means and their sum; one read-back at the end.  The handle's
// state — weights, moving statistics, Adam moments, step count, inference images — is only read.
extern "C" int azr_nn_validate(azr_engine* h, const void* rec265_host, size_t n, int batch_size, float* loss_pi_out, float* loss_v_out,
                               float* rec_loss_pi_host, float* rec_loss_v_host)
{
    ENTER(h);
    if (!h->weights_set) { h->err = "azr_nn_validate: no weights"; return AZR_E_STATE; }
    if ((!rec265_host && n > 0) || batch_size < 2) { h->err = "azr_nn_validate: bad arguments"; return AZR_E_INVALID_ARGUMENT; }
    const size_t nb = n / (size_t)batch_size;   // the remainder is dropped (alphazero_nn.cpp:519)
    if (nb == 0) {   // the reference's 0 / 0
        if (loss_pi_out) *loss_pi_out = NAN;
        if (loss_v_out) *loss_v_out = NAN;
        return AZR_OK;
    }
    if (nb * (size_t)batch_size > (size_t)INT32_MAX) { h->err = "azr_nn_validate: too many records for one call"; return AZR_E_INVALID_ARGUMENT; }
    TRY(ctx_ensure(h, batch_size));
    TrainState* c = ctx_of(h);
    const Slabs& s = *c->slabs;
    hipStream_t st = h->stream;
    const int BS = batch_size, B = c->blocks;
    const size_t nrec = nb * (size_t)BS;
    const size_t need = val_rec(nb, nrec);
    TRY(grow(h, (void**)&c->vbuf, &c->vbuf_cap, need, sizeof(float)));
    ValHdr* hdr = reinterpret_cast<ValHdr*>(c->vbuf);   // (a device address: only its members' addresses are taken here)
    float* means = c->vbuf + val_mean(0);
    float* lossb = c->vbuf + val_rec(nb, 0);
    TRY(upload_records(h, c, rec265_host, nrec));
    std::vector<int> id(nrec);
    for (size_t i = 0; i < nrec; i++) id[i] = (int)i;
    HIPCHK(h, hipMemcpyAsync(c->perm, id.data(), nrec * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemsetAsync(hdr, 0, sizeof(ValHdr), st));
    // once per call: the moving statistics into the statistics slots, the padded stem kernel, the packed forward kernels
    const float* w = h->net.d_flat;
    hipLaunchKernelGGL(t_bn_moving, dim3(c->L + 1), dim3(256), 0, st, w, c->L, c->mean, c->istd, c->hstat);
    hipLaunchKernelGGL(t_stem_pad, grid1((size_t)KS * NF, 256), dim3(256), 0, st, w, c->wpad);
    if (s.plan.sb) {
        const dim3 pg((unsigned)((WPACK / 8 + 255) / 256), 2 * B);
        hipLaunchKernelGGL((t_pack_w<3>), pg, dim3(256), 0, st, w, 0, c->wpf[0], c->wpf[1], c->wpf[2], s.plan.f16 ? FWD_WSCALE : 0.0f, &hdr->range);
    }
    for (size_t k = 0; k < nb; k++) {
        hipLaunchKernelGGL(t_gather, dim3(BS), dim3(64), 0, st, c->rec, c->perm, (const int*)hdr->cur, BS, s.in88, s.pit, s.zt);
        hipLaunchKernelGGL(t_tick_batch, dim3(1), dim3(1), 0, st, hdr->cur, BS);
        TRY(eval_step(h, c, lossb + k * 2 * BS));
    }
    hipLaunchKernelGGL(t_val_means, dim3((unsigned)nb), dim3(256), 0, st, (const float*)lossb, BS, means);
    hipLaunchKernelGGL(t_val_sum, dim3(1), dim3(1), 0, st, (const float*)means, (int)nb, hdr->sum);
    HIPCHK(h, hipGetLastError());
    const bool per_record = rec_loss_pi_host || rec_loss_v_host;
    std::vector<float> out(per_record ? need : val_mean(0));
    HIPCHK(h, hipMemcpyAsync(out.data(), c->vbuf, out.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    ValHdr got;
    memcpy(&got, out.data(), sizeof got);
    if (got.range) {
        h->err = "azr_nn_validate: a conv weight is outside the range of the fp16-pair forward conv (|w| must stay below 64) or is not a number";
        return AZR_E_INVALID_ARGUMENT;
    }
    if (loss_pi_out) *loss_pi_out = got.sum[0] / (float)nb;
    if (loss_v_out) *loss_v_out = got.sum[1] / (float)nb;
    for (size_t i = 0; per_record && i < nrec; i++) {
        if (rec_loss_pi_host) rec_loss_pi_host[i] = out[val_rec(nb, i)];
        if (rec_loss_v_host) rec_loss_v_host[i] = out[val_rec(nb, i) + 1];
    }
    return AZR_OK;
}

// ---- the handle's own RCCL communicator (one process per GPU; the unique id travels by whatever the launcher has: torch.distributed,
//      MPI, a file) ----------------------------------------------------------------------------------------------------------------
extern "C" int azr_dp_unique_id(void* id128)
{
    if (!id128) return AZR_E_INVALID_ARGUMENT;
    RcclApi* R = rccl_api();
    if (!R->lib) return AZR_E_STATE;
    ncclUniqueId id;
    if (R->GetUniqueId(&id) != ncclSuccess) return AZR_E_HIP;
    static_assert(sizeof id == AZR_DP_ID_BYTES, "ncclUniqueId size");
    memcpy(id128, &id, sizeof id);
    return AZR_OK;
}

extern "C" int azr_dp_shutdown(azr_engine* h)
{
    if (!h) return AZR_E_BAD_HANDLE;
    if (h->dp_comm) {
        (void)hipSetDevice(h->cfg.device);
        if (h->stream) (void)hipStreamSynchronize(h->stream);
        rccl_api()->CommDestroy(static_cast<ncclComm_t>(h->dp_comm));
        h->dp_comm = nullptr;
    }
    h->dp_rank = 0; h->dp_world = 0;
    return AZR_OK;
}

namespace azr {
void dp_free(azr_engine* h) { azr_dp_shutdown(h); }
}  // namespace azr

extern "C" int azr_dp_init(azr_engine* h, int rank, int world, const void* id128)
{
    ENTER(h);
    if (!id128 || world < 1 || rank < 0 || rank >= world) { h->err = "azr_dp_init: need 0 <= rank < world and the 128-byte id of azr_dp_unique_id"; return AZR_E_INVALID_ARGUMENT; }
    RcclApi* R = rccl_api();
    if (!R->lib) { h->err = R->err; return AZR_E_STATE; }
    azr_dp_shutdown(h);
    ncclUniqueId id;
    memcpy(&id, id128, sizeof id);
    ncclComm_t comm = nullptr;
    const ncclResult_t rc = R->CommInitRank(&comm, world, id, rank);   // collective over the `world` processes; binds to the current device
    if (rc != ncclSuccess) { h->err = std::string("ncclCommInitRank: ") + R->GetErrorString(rc); return AZR_E_HIP; }
    h->dp_comm = comm; h->dp_rank = rank; h->dp_world = world;
    return AZR_OK;
}

extern "C" int azr_nn_train_grads(azr_engine* h, float* flat_host, size_t count)
{
    ENTER(h);
    TrainState* c = ctx_of(h);
    if (!c) { h->err = "azr_nn_train_grads: no training step has run"; return AZR_E_STATE; }
    if (!flat_host || count != c->count) return AZR_E_INVALID_ARGUMENT;
    HIPCHK(h, hipMemcpy(flat_host, c->g, count * sizeof(float), hipMemcpyDeviceToHost));
    return AZR_OK;
}

extern "C" int azr_nn_train_reset(azr_engine* h)
{
    if (!h) return AZR_E_BAD_HANDLE;
    azr::train_free(h);
    return AZR_OK;
}

extern "C" void azr_default_train_options(azr_train_options* o)
{
    if (o) *o = TRAIN_OPT_DEFAULT;
}

extern "C" int azr_nn_train_set_options(azr_engine* h, const azr_train_options* o)
{
    if (!h) return AZR_E_BAD_HANDLE;
    if (!o) { h->err = "azr_nn_train_set_options: no options"; return AZR_E_INVALID_ARGUMENT; }
    const char* why = nullptr;
    for (float x : {o->lr, o->l2, o->decay_gamma, o->lr_min, o->clip_norm, o->ema_decay})
        if (!std::isfinite(x)) why = "a value is not finite";
    if (why) {}
    else if (!(o->lr > 0.0f)) why = "lr must be > 0";
    else if (o->l2 < 0.0f) why = "l2 must be >= 0";
    else if (o->lr_schedule != AZR_LR_CONSTANT && o->lr_schedule != AZR_LR_COSINE && o->lr_schedule != AZR_LR_STEP) why = "unknown lr_schedule";
    else if (o->warmup_steps < 0) why = "warmup_steps must be >= 0";
    else if (o->lr_schedule == AZR_LR_COSINE && o->total_steps <= o->warmup_steps) why = "COSINE needs total_steps > warmup_steps";
    else if (o->lr_schedule == AZR_LR_COSINE && (o->lr_min < 0.0f || o->lr_min > o->lr)) why = "COSINE needs lr_min in [0, lr]";
    else if (o->lr_schedule == AZR_LR_STEP && o->decay_period < 1) why = "STEP needs decay_period >= 1";
    else if (o->lr_schedule == AZR_LR_STEP && (o->decay_gamma <= 0.0f || o->decay_gamma > 1.0f)) why = "STEP needs decay_gamma in (0, 1]";
    else if (o->clip_norm < 0.0f) why = "clip_norm must be 0 (off) or > 0";
    else if (o->ema_decay < 0.0f || o->ema_decay >= 1.0f) why = "ema_decay must be 0 (off) or in (0, 1)";
    if (why) { h->err = std::string("azr_nn_train_set_options: ") + why + "; the previous options stay in force"; return AZR_E_INVALID_ARGUMENT; }
    h->train_opt = *o;
    return AZR_OK;
}

extern "C" int azr_nn_train_get_options(azr_engine* h, azr_train_options* o)
{
    if (!h) return AZR_E_BAD_HANDLE;
    if (!o) { h->err = "azr_nn_train_get_options: no destination"; return AZR_E_INVALID_ARGUMENT; }
    *o = h->train_opt;
    return AZR_OK;
}

extern "C" int azr_nn_train_stats(azr_engine* h, azr_train_stats* out)
{
    ENTER(h);
    TrainState* c = ctx_of(h);
    if (!c || c->step == 0) { h->err = "azr_nn_train_stats: no training step has run"; return AZR_E_STATE; }
    if (!out) { h->err = "azr_nn_train_stats: no destination"; return AZR_E_INVALID_ARGUMENT; }
    StatRow row;
    float lr_t = 0.0f;
    HIPCHK(h, hipMemcpy(&row, c->row, sizeof row, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(&lr_t, c->lr, sizeof lr_t, hipMemcpyDeviceToHost));
    out->step = c->step;
    out->lr = c->last_default ? LR : row.lr;
    out->lr_t = lr_t;
    out->grad_norm = c->last_default ? NAN : row.norm;
    out->clip_scale = c->last_default ? 1.0f : row.scale;
    out->clipped_steps = row.clipped;
    out->ema_steps = c->ema_steps;
    return AZR_OK;
}

extern "C" int azr_nn_get_ema_weights(azr_engine* h, float* flat_host, size_t count)
{
    ENTER(h);
    TrainState* c = ctx_of(h);
    if (!c || !c->e) { h->err = "azr_nn_get_ema_weights: there is no EMA vector (no step has run with ema_decay > 0 since the optimiser state was created)"; return AZR_E_STATE; }
    if (!flat_host || count != c->count) { h->err = "azr_nn_get_ema_weights: count must be azr_nn_param_count"; return AZR_E_INVALID_ARGUMENT; }
    HIPCHK(h, hipMemcpy(flat_host, c->e, count * sizeof(float), hipMemcpyDeviceToHost));
    return AZR_OK;
}

