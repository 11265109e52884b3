// azr_net_bf16.hip — k_tower_bf16<1>, the one-board tower: the residual tower of python/src/build_graph.py:63-74 as ONE persistent
// MFMA kernel (gfx950) per board, bf16 or fp16 (El<F16>); and the host side of every bf16 / fp16 tower: weight packing, the tile plan
// (plan_sb) and the launches.
//
// Launches of 129..256 boards run this kernel, and it is the guarded recompute queued behind every k_tower_sc launch
// (azr_tower_sc.hip).  Written independently of the multi-board tiles (k_tower_sb, k_tower_sc), it is the reference they are compared
// with bit for bit (AZR_TOWER_SB=0 / AZR_TOWER_SC=0): its tables, stem and epilogue are its own, and of what the towers share it takes the
// element type, the packed layout and the fused heads (azr_bf16_common.hpp) only, nothing of azr_tower_common.hpp.
//   * A workgroup (8 waves, 512 threads, two per CU) owns one board for the ENTIRE stem + 2B conv layers: 42 cells -> M = 48 GEMM
//     rows (row = cell, rows 42..47 are zero pad rows).  The activations never leave LDS: two ping-pong images [48 rows + 1 zero
//     row][256 + 16 pad] bf16.  HBM sees the 88-byte input, the weights, and 45 floats out.
//   * Implicit GEMM per layer: M = board cells, N = 256 output channels, K = 9 taps x 256 input channels, on
//     v_mfma_f32_16x16x32_bf16 / _f16 (fp32 accumulate).  The activation operand of tap (dy,dx) is the SAME LDS image read at a
//     per-lane row offset (out-of-board neighbours read the zero row) — no im2col, no halo copies.
//   * Waves split N (32 channels = two 16-wide tiles each), so weight fragments are private to a wave and stream
//     global -> VGPR with no LDS staging, pre-packed on the host in exactly the lane order of the MFMA operand (one coalesced
//     1-KiB global_load_dwordx4 per fragment), through a ring of two taps (16 k-steps) that never drains.
//   * Weights are the MFMA "A" operand, activations "B": D = [channel][cell], so a lane ends up with 4 consecutive channels of
//     one cell.  Epilogue per layer in registers: folded BN (fp32 scale/shift), residual add (read from the LDS image being
//     replaced), ReLU, round-to-nearest-even, written straight back into LDS with one 8-byte store per tile.
//   * conv_bn of the stem normalises over the board ROW (build_graph.py:68 axis=1): per-row scale/shift.
// One barrier per layer.  The heads (fused_heads, azr_bf16_common.hpp) run at the end of the same launch on the LDS-resident tower
// output: one kernel = one whole net forward.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "azr_internal.hpp"
#include "azr_bf16_common.hpp"

using namespace azr;

namespace {
constexpr int THREADS = 512, NT = 2, WCOLS = NT * 16;   // 8 waves x 2 column tiles of 16 channels
constexpr int ROWS = 42, MT = 3, ZR = MT * 16;          // board cells, M tiles, index of the zero row (rows ROWS .. ZR - 1: pad rows)
constexpr int RING = 2 * KS_PER_TAP;                    // weight ring depth in k-steps
// LDS map (dynamic)
constexpr int BUF = (ZR + 1) * ROWB;            // one activation image incl. its zero row
constexpr int IN88_OFF = 2 * BUF;               // 96 B NNInputData image
constexpr int ROWOF_OFF = IN88_OFF + 96;        // u8 [42 (+ pad to 128)]: cell -> row
constexpr int ROWCELL_OFF = ROWOF_OFF + 128;    // u16 [ZR]: row -> y | x << 4, 0xffff = pad
constexpr int LDS_BYTES = ROWCELL_OFF + 2 * ZR;

// LDS row a lane reads for cell info `ri` (y | x << 4; 0xffff for a pad row) under tap (dy,dx); taps outside the board read the
// zero row
__device__ __forceinline__ int tap_row(int ri, int dy, int dx, const uint8_t* __restrict__ rowof)
{
    const int y = (ri & 15) + dy, x = ((ri >> 4) & 15) + dx;
    const bool ok = (unsigned)y < 7u && (unsigned)x < 6u;
    const int r = rowof[ok ? y * 6 + x : 0];
    return ok ? r : ZR;
}

// one tap = 8 k-steps against ring slots SB .. SB+7.  `wb` is the wave-UNIFORM byte pointer to the current
// k-step's 16-KiB fragment block (advanced with scalar adds); `loff` is this lane's byte offset inside a block.
template <int SB, bool F16>
__device__ __forceinline__ void conv_tap(const uint8_t* IN, int tap, const char* __restrict__& wb, uint32_t loff, s16x8 (&bq)[RING][NT],
                                         f32x4 (&acc)[MT][NT], s16x8 (&a)[2][MT], int (&aoff)[MT], const int (&rinfo)[MT], int g16,
                                         const uint8_t* __restrict__ rowof)
{
    const int ntap = tap < 8 ? tap + 1 : 8;
    const int ndy = ntap / 3 - 1, ndx = ntap % 3 - 1;
    int noff[MT];
#pragma unroll
    for (int ks = 0; ks < KS_PER_TAP; ks++) {
        const int cur = ks & 1, nxt = cur ^ 1;
        if (ks == KS_PER_TAP - 2) {  // the next tap's rows, one k-step before they are needed (short live range)
#pragma unroll
            for (int mt = 0; mt < MT; mt++) noff[mt] = tap_row(rinfo[mt], ndy, ndx, rowof) * ROWB + g16;
        }
        // (1) LDS reads of the NEXT k-step's activation fragments go out first ...
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            if (ks < KS_PER_TAP - 1) a[nxt][mt] = *reinterpret_cast<const s16x8*>(IN + aoff[mt] + (ks + 1) * 64);
            else a[nxt][mt] = *reinterpret_cast<const s16x8*>(IN + noff[mt]);
        }
        __builtin_amdgcn_sched_barrier(0);
        // (2) ... and fly under this k-step's MFMAs; then the freed ring slot is refilled one ring ahead
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int nt = 0; nt < NT; nt++)
                // D[channel][cell]: row = 4*(lane>>4)+j = channel, col = lane&15 = board cell
                acc[mt][nt] = El<F16>::mfma(bq[SB + ks][nt], a[cur][mt], acc[mt][nt]);
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
            bq[SB + ks][nt] = *reinterpret_cast<const s16x8*>(wb + RING * KBYTES + loff + nt * 1024);
        wb += KBYTES;
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int mt = 0; mt < MT; mt++) aoff[mt] = noff[mt];
}

// One 3x3 conv layer F->F: acc[mt][nt] = sum over 9 taps x 256 channels (72 k-steps of 32).
// Weight fragments come from a RING of 16 k-steps held in VGPRs that never drains: the packed tower weights of
// all layers are one contiguous stream in exactly consumption order, so a slot is refilled with the k-step one ring
// ahead right after its MFMAs issue — also across layer boundaries, where the epilogue + barrier then overlap the
// next layer's weight latency.  Activation fragments are double-buffered one k-step ahead so their LDS latency hides under
// the current MFMAs; scheduling regions (sched_barrier) keep that order.
// PAR = parity of the layer's first tap in the global tap sequence (9 taps per layer: it alternates per layer).
template <int PAR, bool F16>
__device__ __forceinline__ void conv_tower_layer(const uint8_t* IN, const char* __restrict__& wb, uint32_t loff, s16x8 (&bq)[RING][NT],
                                                 f32x4 (&acc)[MT][NT], const int (&rinfo)[MT], int g16, const uint8_t* __restrict__ rowof,
                                                 const float* __restrict__ fs, float4 (&sc)[NT], float4 (&sh)[NT])
{
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) acc[mt][nt] = f32x4{0, 0, 0, 0};
    int aoff[MT];
    s16x8 a[2][MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        aoff[mt] = tap_row(rinfo[mt], -1, -1, rowof) * ROWB + g16;
        a[0][mt] = *reinterpret_cast<const s16x8*>(IN + aoff[mt]);
    }
    constexpr int S0 = PAR ? 8 : 0, S1 = PAR ? 0 : 8;
    for (int tap = 0; tap < 8; tap += 2) {
        conv_tap<S0, F16>(IN, tap, wb, loff, bq, acc, a, aoff, rinfo, g16, rowof);
        conv_tap<S1, F16>(IN, tap + 1, wb, loff, bq, acc, a, aoff, rinfo, g16, rowof);
    }
    // this layer's folded BN (4 consecutive channels per lane and tile) is requested one tap before the epilogue:
    // early enough not to wait behind the weight ring, late enough not to hold 16 VGPRs through the layer
#pragma unroll
    for (int nt = 0; nt < NT; nt++) {
        sc[nt] = *reinterpret_cast<const float4*>(fs + nt * 16);
        sh[nt] = *reinterpret_cast<const float4*>(fs + NF + nt * 16);
    }
    conv_tap<S0, F16>(IN, 8, wb, loff, bq, acc, a, aoff, rinfo, g16, rowof);
}

// the whole network for board blockIdx.x
template <bool F16>
__global__ __launch_bounds__(THREADS, 2) void k_tower_bf16(const uint8_t* __restrict__ in88, int in_stride, int n,
                                                            const uint16_t* __restrict__ stem_wp, const uint16_t* __restrict__ tower_wp,
                                                            const float* __restrict__ fold, int blocks, const float* __restrict__ hp,
                                                            float* __restrict__ pi_out, float* __restrict__ v_out,
                                                            unsigned long long* __restrict__ diag, const int* __restrict__ slot_map,
                                                            unsigned* __restrict__ guard, const int* __restrict__ n_dev, unsigned tag)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int board0 = blockIdx.x;
    // guard != null: this launch stands behind a k_tower_sc launch of the same batch and runs only if that one raised its give-up word
    // (1: a hand-off ran out of polls, its results are garbage; 2: more boards than it takes) — every workgroup ends here otherwise;
    // workgroup 0 counts the recompute of a launch that gave up
    // (the word holds (serial of the launch << 2) | reason; tag = this launch pair's serial << 2).  Workgroup 0 also zeroes the pairs' arrival
    // counters and XCC words for the next k_tower_sc launch — this kernel is what runs between two of them in stream order.
    if (guard) {
        if (board0 == 0 && threadIdx.x < SC_W_GIVEUP) guard[threadIdx.x] = 0u;
        const unsigned word = (unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(guard + SC_W_GIVEUP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        const int why = (word ^ tag) < 4u ? (int)(word & 3u) : 0;
        if (why == 0) return;
        if (why == 1 && board0 == 0 && threadIdx.x == 0) __hip_atomic_fetch_add(guard + SC_W_FALLBACKS, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // n_dev != null: the batch size is a word in device memory, the grid covers the largest batch
    if (n_dev) {
        n = __builtin_amdgcn_readfirstlane(*n_dev);
        if (board0 >= n) return;
    }
    uint8_t* bufX = lds;
    uint8_t* bufT = lds + BUF;
    uint8_t* in_l = lds + IN88_OFF;
    uint8_t* rowof = lds + ROWOF_OFF;                                        // cell -> row
    uint16_t* rowcell = reinterpret_cast<uint16_t*>(lds + ROWCELL_OFF);      // row -> y | x << 4
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = lane & 15, g = lane >> 4;
    // clock diagnostic (azr_debug_tower_clock): shader-clock and 100 MHz real-time stamps around the whole tower of
    // workgroup 0; `diag` is null in every product launch
    if (diag && blockIdx.x == 0 && tid == 0) { diag[0] = __builtin_amdgcn_s_memtime(); diag[1] = __builtin_amdgcn_s_memrealtime(); }

    // ---- stage the NNInputData image, zero the pad rows and the zero row, fill the row tables
    if (tid < 96) {
        // slot_map (optional): board i of this launch is leaf slot slot_map[i] (two-net arena: each net sees its own leaves)
        const int slot = board0 < n ? (slot_map ? slot_map[board0] : board0) : 0;
        in_l[tid] = (board0 < n && tid < 88) ? in88[(size_t)slot * in_stride + tid] : (uint8_t)0;
    }
    // (the pad rows' accumulator rows are never stored, but they are MFMA operands)
    for (int i = tid; i < (ZR + 1 - ROWS) * (ROWB / 4); i += THREADS) {
        reinterpret_cast<uint32_t*>(bufX + ROWS * ROWB)[i] = 0;
        reinterpret_cast<uint32_t*>(bufT + ROWS * ROWB)[i] = 0;
    }
    if (tid < ZR) {
        if (tid < ROWS) rowof[tid] = (uint8_t)tid;
        rowcell[tid] = tid < ROWS ? (uint16_t)((tid / 6) | ((tid % 6) << 4)) : (uint16_t)0xffffu;
    }
    __syncthreads();
    // stem features: bufT as [ZR + 1][16] bf16 (row ZR = zero row); planes 13..15 are zero
    for (int i = tid; i < (ZR + 1) * 16; i += THREADS) {
        const int r = i >> 4, c = i & 15;
        float v = 0.0f;
        const int ci = r < ZR ? rowcell[r] : 0xffff;
        if (ci != 0xffff) v = plane_value(in_l, (ci & 15) * 6 + ((ci >> 4) & 15), c);
        reinterpret_cast<uint16_t*>(bufT)[i] = El<F16>::rne(v);
    }
    __syncthreads();

    // ---- per-lane geometry of the rows (= cells) this lane feeds as MFMA operand (row = mt*16 + m)
    int rinfo[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) rinfo[mt] = rowcell[mt * 16 + m];   // 0xffff (y = x = 15) for a pad row
    f32x4 acc[MT][NT];

    // ---- start the weight ring: the first ring of k-steps of layer 0 flies while the stem runs
    const char* __restrict__ wb = reinterpret_cast<const char*>(tower_wp);      // wave-uniform, scalar-advanced
    const uint32_t loff = (uint32_t)((wave * NT) * 64 + lane) * 16u;             // this lane's fragment bytes in a k-step
    s16x8 bq[RING][NT];
#pragma unroll
    for (int ks = 0; ks < RING; ks++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) bq[ks][nt] = *reinterpret_cast<const s16x8*>(wb + ks * KBYTES + loff + nt * 1024);

    // ---- stem: 3x3 conv 13 -> 256, two taps per 32-deep k-step (tap slot = 2*ks + (g >> 1), channels (g & 1)*8 ..)
    {
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int nt = 0; nt < NT; nt++) acc[mt][nt] = f32x4{0, 0, 0, 0};
        const s16x8* wp = reinterpret_cast<const s16x8*>(stem_wp) + (size_t)(wave * NT) * 64 + lane;
#pragma unroll
        for (int ks = 0; ks < STEM_KS; ks++) {
            const int tap = 2 * ks + (g >> 1);
            const int dy = tap / 3 - 1, dx = tap % 3 - 1;
            s16x8 b[NT];
#pragma unroll
            for (int nt = 0; nt < NT; nt++) b[nt] = wp[(size_t)ks * FRAGS_PER_KSTEP * 64 + nt * 64];
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                const int row = tap < 9 ? tap_row(rinfo[mt], dy, dx, rowof) : ZR;
                const s16x8 av = *reinterpret_cast<const s16x8*>(bufT + row * FROWB + (g & 1) * 16);
#pragma unroll
                for (int nt = 0; nt < NT; nt++) acc[mt][nt] = El<F16>::mfma(b[nt], av, acc[mt][nt]);
            }
        }
        // conv_bn over the board row + ReLU -> bufX.  D layout: col = lane & 15 = board cell, row = 4*(lane>>4)+j = channel
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            const int r = mt * 16 + m;
            if (rinfo[mt] != 0xffff) {
                const int y = rinfo[mt] & 15;
                const float sc = fold[y], sh = fold[7 + y];
#pragma unroll
                for (int nt = 0; nt < NT; nt++) {
                    const int c0 = wave * WCOLS + nt * 16 + g * 4;
                    uint16_t o4[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const float v = fmaf(acc[mt][nt][j], sc, sh);
                        o4[j] = El<F16>::rne(v > 0.0f ? v : 0.0f);
                    }
                    *reinterpret_cast<uint2*>(bufX + r * ROWB + c0 * 2) = uint2{(uint32_t)o4[0] | ((uint32_t)o4[1] << 16), (uint32_t)o4[2] | ((uint32_t)o4[3] << 16)};
                }
            }
        }
    }
    __syncthreads();

    // ---- residual tower: 2 conv layers per block, activations resident in LDS
    const int g16 = g * 16;
    auto epilogue = [&](bool second, uint8_t* OUT, const float4 (&sc)[NT], const float4 (&sh)[NT]) {
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            const int r = mt * 16 + m;
            if (r < ROWS) {
#pragma unroll
                for (int nt = 0; nt < NT; nt++) {
                    uint2* o = reinterpret_cast<uint2*>(OUT + r * ROWB + (wave * WCOLS + nt * 16 + g * 4) * 2);
                    const float4 s4 = sc[nt], h4 = sh[nt];
                    float v0 = fmaf(acc[mt][nt][0], s4.x, h4.x), v1 = fmaf(acc[mt][nt][1], s4.y, h4.y);
                    float v2 = fmaf(acc[mt][nt][2], s4.z, h4.z), v3 = fmaf(acc[mt][nt][3], s4.w, h4.w);
                    if (second) {  // shortcut: OUT still holds the block's input at these 4 channels of this cell
                        const uint2 x = *o;
                        v0 += El<F16>::tof((uint16_t)(x.x & 0xffffu)); v1 += El<F16>::tof((uint16_t)(x.x >> 16));
                        v2 += El<F16>::tof((uint16_t)(x.y & 0xffffu)); v3 += El<F16>::tof((uint16_t)(x.y >> 16));
                    }
                    const uint32_t lo = (uint32_t)El<F16>::rne(v0 > 0.0f ? v0 : 0.0f) | ((uint32_t)El<F16>::rne(v1 > 0.0f ? v1 : 0.0f) << 16);
                    const uint32_t hi = (uint32_t)El<F16>::rne(v2 > 0.0f ? v2 : 0.0f) | ((uint32_t)El<F16>::rne(v3 > 0.0f ? v3 : 0.0f) << 16);
                    *o = uint2{lo, hi};
                }
            }
        }
    };
    for (int blk = 0; blk < blocks; blk++) {
        float4 sc[NT], sh[NT];
        const float* fs = fold + 14 + (size_t)(2 * blk) * 2 * NF + wave * WCOLS + g * 4;
        conv_tower_layer<0, F16>(bufX, wb, loff, bq, acc, rinfo, g16, rowof, fs, sc, sh);
        epilogue(false, bufT, sc, sh);
        __syncthreads();
        conv_tower_layer<1, F16>(bufT, wb, loff, bq, acc, rinfo, g16, rowof, fs + 2 * NF, sc, sh);
        epilogue(true, bufX, sc, sh);
        __syncthreads();
    }

    if (diag && blockIdx.x == 0 && tid == 0) { diag[2] = __builtin_amdgcn_s_memtime(); diag[3] = __builtin_amdgcn_s_memrealtime(); }
    // ---- both heads on the tower output in bufX; bufT is free: the head features at its start, the 1x1-conv weight columns behind them
    fused_heads<1, THREADS>(tid, hp, reinterpret_cast<float*>(bufT + 8192), reinterpret_cast<float*>(bufT), rowof, ImageAct<F16>{bufX}, board0, n,
                            slot_map, pi_out, v_out);
}

Bf16Net* bn(azr_engine* h) { return bf16net(h); }
}  // namespace

namespace azr {

int net_bf16_alloc(azr_engine* h)
{
    Bf16Net* x = new Bf16Net();
    h->net.bf16ctx = x;
    const int B = h->net.blocks;
    x->f16 = h->cfg.net_dtype == AZR_NET_F16;
    if (x->f16) HIPCHK(h, hipMalloc((void**)&x->fold16, (14 + (size_t)2 * B * 2 * NF) * sizeof(float)));
    HIPCHK(h, hipMalloc((void**)&x->stem_wp, STEM_HALFS * 2));
    HIPCHK(h, hipMalloc((void**)&x->tower_wp, tower_stream_bytes(B)));  // + ring run-off
    HIPCHK(h, hipMemsetAsync(x->tower_wp, 0, tower_stream_bytes(B), h->stream));
    HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(k_tower_bf16<false>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
    HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(k_tower_bf16<true>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
    // test hooks (libazr_hip_test.so only, azr_internal.hpp; read ONCE, here, never in the launch path): AZR_TOWER_SB = 0: k_tower_bf16<1>
    // (one board per workgroup) for every launch — the independently written implementation the single-image tiles are compared
    // with bit for bit; 1 (default, and the product): plan; 2 / 3 / 4: force the 4- / 2- / 3-board single-image tile
    x->sb_mode = hook_env_int("AZR_TOWER_SB", 1);
    // AZR_TOWER_SC=0: launches of <= 128 boards on k_tower_bf16<1> instead of the split-channel tower (A/B measurements, tests)
    x->sc_mode = hook_env_int("AZR_TOWER_SC", 1);
    int rc = tower_sc_init(h);
    if (rc) return rc;
    return tower_sb_init(h);
}

void net_bf16_free(azr_engine* h)
{
    if (!h->net.bf16ctx) return;
    Bf16Net* x = bn(h);
    tower_sc_free(h);
    if (x->stem_wp) hipFree(x->stem_wp);
    if (x->tower_wp) hipFree(x->tower_wp);
    if (x->fold16) hipFree(x->fold16);
    delete x;
    h->net.bf16ctx = nullptr;
}

// pack the HWIO fp32 kernels of the AZRW vector into MFMA B-operand fragment order (bf16 or fp16, RNE):
// fragment (layer, tap, ks, wave, nt), lane l, element j  <-  W[tap][ci = ks*32 + 8*(l>>4) + j][co = wave*32 + nt*16 + (l&15)]

// power-of-two scale of one fp16-packed weight tensor: max |2^e w| in [2^13, 2^14) (e clipped to [-2, 24]); false = a weight is
// outside the fp16 range or not a number
static bool f16_scale(const float* W, size_t n, int& e)
{
    float worst = 0.0f;
    for (size_t i = 0; i < n; i++) {
        const float aw = W[i] < 0 ? -W[i] : W[i];
        if (!(aw <= worst)) worst = aw;   // (also catches NaN)
    }
    if (!(worst < 65504.0f)) return false;
    e = 0;
    if (worst > 0.0f) {
        int we;
        frexpf(worst, &we);           // worst = f * 2^we, f in [0.5, 1)
        e = 14 - we;
        if (e > 24) e = 24;
        if (e < -2) e = -2;
    }
    return true;
}
static inline uint16_t f2h(float f) { const _Float16 v = (_Float16)f; uint16_t u; memcpy(&u, &v, 2); return u; }

// packs the stem and tower conv weights into MFMA fragments: bf16 (NET_BF16), or fp16 of 2^k w with k per layer and 2^-k folded into
// the layer's BN scale (NET_F16; `fold_host` = the fp32 fold of net_upload)
int net_bf16_upload(azr_engine* h, const float* fold_host)
{
    Bf16Net* x = bn(h);
    const int B = h->net.blocks;
    const bool f16 = x->f16;
    const float* flat = h->flat.data();
    std::vector<uint16_t> stem(STEM_HALFS, 0), tower((size_t)2 * B * TOWER_LAYER_HALFS);
    std::vector<float> fold(fold_host, fold_host + 14 + (size_t)2 * B * 2 * NF);
    float sS = 1.0f;
    if (f16) {
        int e = 0;
        if (!f16_scale(flat, (size_t)9 * 13 * NF, e)) { h->err = "NET_F16: a stem weight is outside the fp16 range (|w| must be < 65504) or not a number"; return AZR_E_INVALID_ARGUMENT; }
        sS = ldexpf(1.0f, e);
        for (int y = 0; y < 7; y++) fold[y] *= ldexpf(1.0f, -e);
    }
    for (int ks = 0; ks < STEM_KS; ks++)
        for (int w = 0; w < 8; w++)
            for (int nt = 0; nt < 2; nt++)
                for (int l = 0; l < 64; l++)
                    for (int j = 0; j < 8; j++) {
                        const int g = l >> 4, tap = 2 * ks + (g >> 1), ch = (g & 1) * 8 + j, co = w * 32 + nt * 16 + (l & 15);
                        float v = (tap < 9 && ch < 13) ? flat[((size_t)tap * 13 + ch) * NF + co] : 0.0f;
                        stem[((((size_t)ks * 8 + w) * 2 + nt) * 64 + l) * 8 + j] = f16 ? f2h(v * sS) : f2bf(v);
                    }
    const size_t layer_floats = (size_t)9 * NF * NF + 4 * NF;
    const float* t0 = flat + 9 * 13 * NF + 28;
    for (int L = 0; L < 2 * B; L++) {
        const float* W = t0 + (size_t)L * layer_floats;
        float sL = 1.0f;
        if (f16) {
            int e = 0;
            if (!f16_scale(W, (size_t)9 * NF * NF, e)) { h->err = "NET_F16: a conv weight is outside the fp16 range (|w| must be < 65504) or not a number"; return AZR_E_INVALID_ARGUMENT; }
            sL = ldexpf(1.0f, e);
            float* fs = fold.data() + 14 + (size_t)L * 2 * NF;
            for (int i = 0; i < NF; i++) fs[i] *= ldexpf(1.0f, -e);
        }
        uint16_t* dst = tower.data() + (size_t)L * TOWER_LAYER_HALFS;
        for (int tap = 0; tap < 9; tap++)
            for (int ks = 0; ks < 8; ks++)
                for (int w = 0; w < 8; w++)
                    for (int nt = 0; nt < 2; nt++)
                        for (int l = 0; l < 64; l++) {
                            const int ci0 = ks * 32 + 8 * (l >> 4), co = w * 32 + nt * 16 + (l & 15);
                            uint16_t* d = dst + (((((size_t)tap * 8 + ks) * 8 + w) * 2 + nt) * 64 + l) * 8;
                            for (int j = 0; j < 8; j++) {
                                const float wv = W[((size_t)tap * NF + ci0 + j) * NF + co];
                                d[j] = f16 ? f2h(wv * sL) : f2bf(wv);
                            }
                        }
    }
    HIPCHK(h, hipMemcpyAsync(x->stem_wp, stem.data(), stem.size() * 2, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(x->tower_wp, tower.data(), tower.size() * 2, hipMemcpyHostToDevice, h->stream));
    if (f16) HIPCHK(h, hipMemcpyAsync(x->fold16, fold.data(), fold.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return AZR_OK;
}

// Single-image tiles (azr_tower_sb.hip) for 2, 3 or 4 boards per workgroup: boards per workgroup for a launch of n boards, or
// 0 = none of them (k_tower_sc or k_tower_bf16<1>).  AZR_TOWER_SB: 0 = never, 1 = plan (default), 2 / 3 / 4 = force the 4- / 2- /
// 3-board tile for every launch (tests, measurements).
static int plan_sb(int sb_mode, int n)
{
    int snb = sb_mode == 2 ? 4 : sb_mode == 3 ? 2 : sb_mode == 4 ? 3 : 0;
    if (sb_mode == 1 && n > 256) {
        // Relative time of one 256-workgroup round of 2 / 3 / 4 boards per workgroup.  One workgroup per CU is resident, so a launch
        // of w workgroups takes ceil(w / 256) rounds, and only the RATIOS of the round times enter the choice: the three tiles are
        // the same MFMA-bound code, so a box that clocks lower stretches all three alike.  The ratios are those of the tiles'
        // measured shader cycles per workgroup (1.126 / 1.414 / 1.903 M cycles, profiles/tower_boundary_timing.txt;
        // launch times there 0.568 / 0.724 / 0.955 ms).  Before the 4-board tile lost its LDS residual slots the ratios were
        // 0.575 / 0.730, and launch times on three boxes of the pool (1.77 - 2.0 GHz sustained) — 0.61 / 0.80 / 1.05 ms, 0.63 / 0.82 / 1.07
        // and 0.68 / 0.89 / 1.18 — gave the same ratios to 2 %: far inside the margins the plan turns on (the closest call, 768 boards:
        // 3 x 256 at 0.74 against 2 rounds of 2-board tiles at 1.18; the two sets of ratios choose alike up to 10 752 boards).
        static const float T[5] = {0.0f, 0.0f, 0.590f, 0.743f, 1.0f};
        float best = 0.0f;
        for (int c = 4; c >= 2; c--) {
            const int w = (n + c - 1) / c;
            const float t = (float)((w + 255) / 256) * T[c];
            if (snb == 0 || t < best) { snb = c; best = t; }
        }
    }
    return n >= snb ? snb : 0;
}

int net_bf16_forward(azr_engine* h, const uint8_t* d_in88, int in_stride, int n, float* d_pi, float* d_v, const int* d_map, hipStream_t st)
{
    Bf16Net* x = bn(h);
    const float* fold = net_fold(h);
    const int B = h->net.blocks;
    if (h->pe_tower0) hipEventRecord(h->pe_tower0, st);
    if (const int snb = plan_sb(x->sb_mode, n)) {   // more than 256 boards: 2, 3 or 4 per workgroup in one LDS image (azr_tower_sb.hip)
        int rc = tower_sb_launch(h, snb, (n + snb - 1) / snb, d_in88, in_stride, n, d_pi, d_v, d_map, st);
        if (h->pe_tower1) hipEventRecord(h->pe_tower1, st);
        return rc;
    }
    unsigned* guard = nullptr;
    if (x->sb_mode != 0 && x->sc_mode != 0 && n <= 128) {   // up to 128 boards: a board pair's channels split over 4 workgroups (azr_tower_sc.hip)
        int rc = tower_sc_launch(h, d_in88, in_stride, n, d_pi, d_v, d_map, st);
        if (h->pe_tower1) hipEventRecord(h->pe_tower1, st);
        if (rc) return rc;
        // ... and right behind it, in stream order, the one-board-per-workgroup kernel under the launch's give-up word: it recomputes the
        // batch if (and only if) a hand-off of the persistent launch ran out of polls; otherwise its n workgroups end at their first
        // instruction.  Later tree steps on this stream therefore never see the garbage of a launch that gave up.
        guard = x->sc_counters;
    }
    // AZR_TOWER_SB=0 / AZR_TOWER_SC=0: one board per workgroup for the whole net, two ping-pong images, 8 waves x 32 channels
    if (x->f16)
        hipLaunchKernelGGL(k_tower_bf16<true>, dim3(n), dim3(THREADS), LDS_BYTES, st, d_in88, in_stride, n, x->stem_wp, x->tower_wp,
                           (const float*)x->fold16, B, net_head_params(h), d_pi, d_v, x->diag, d_map, guard, nullptr, x->sc_tag);
    else
        hipLaunchKernelGGL(k_tower_bf16<false>, dim3(n), dim3(THREADS), LDS_BYTES, st, d_in88, in_stride, n, x->stem_wp, x->tower_wp, fold, B,
                           net_head_params(h), d_pi, d_v, x->diag, d_map, guard, nullptr, x->sc_tag);
    if (h->pe_tower1 && !guard) hipEventRecord(h->pe_tower1, st);
    HIPCHK(h, hipGetLastError());
    return AZR_OK;
}

// Small batches whose size only the device knows (the arena's and the emptying self-play tail's waiting leaves, counted by the tree step
// into *n_dev ahead of this call in stream order): no read-back, no host synchronisation per pass.  Both launches are sized for n_max
// (<= 256) boards and read the count themselves: the split-channel tower takes up to 128 boards, above that — or when the launch of another
// network beside it (n_other: that one's count, other_wgpp: its workgroups per board pair) leaves it no CU per workgroup — it raises the give-up word with the value 2 and the guarded
// one-board-per-workgroup launch computes the batch; a count of 0 ends every workgroup at once.
bool net_bf16_counted_ok(azr_engine* h, int n_max)
{
    Bf16Net* x = bn(h);
    return x && x->sb_mode == 1 && x->sc_mode != 0 && n_max >= 1 && n_max <= 256;   // the product's plan (no forced tile of the test build)
}

int net_bf16_forward_counted(azr_engine* h, const uint8_t* d_in88, int in_stride, int n_max, const int* n_dev, const int* n_other, int other_wgpp,
                             float* d_pi, float* d_v, const int* d_map, hipStream_t st)
{
    if (!net_bf16_counted_ok(h, n_max) || !n_dev) { h->err = "net_bf16_forward_counted: 1..256 boards on the split-channel tower"; return AZR_E_INVALID_ARGUMENT; }
    Bf16Net* x = bn(h);
    const int B = h->net.blocks;
    if (h->pe_tower0) hipEventRecord(h->pe_tower0, st);
    int rc = tower_sc_launch(h, d_in88, in_stride, n_max, d_pi, d_v, d_map, st, n_dev, n_other, other_wgpp);
    if (h->pe_tower1) hipEventRecord(h->pe_tower1, st);
    if (rc) return rc;
    if (x->f16)
        hipLaunchKernelGGL(k_tower_bf16<true>, dim3(n_max), dim3(THREADS), LDS_BYTES, st, d_in88, in_stride, n_max, x->stem_wp, x->tower_wp,
                           (const float*)x->fold16, B, net_head_params(h), d_pi, d_v, (unsigned long long*)nullptr, d_map, x->sc_counters, n_dev, x->sc_tag);
    else
        hipLaunchKernelGGL(k_tower_bf16<false>, dim3(n_max), dim3(THREADS), LDS_BYTES, st, d_in88, in_stride, n_max, x->stem_wp, x->tower_wp,
                           net_fold(h), B, net_head_params(h), d_pi, d_v, (unsigned long long*)nullptr, d_map, x->sc_counters, n_dev, x->sc_tag);
    HIPCHK(h, hipGetLastError());
    return AZR_OK;
}


}  // namespace azr

// Diagnostics (not part of the product path).  azr_debug_tower_clock: sustained shader clock of the tower kernel under load
// = d(s_memtime) / d(s_memrealtime) x 100 MHz around workgroup 0's whole tower, after `warm` back-to-back launches on the
// leaf buffers.  azr_debug_tower_trace: per workgroup of that launch (k_tower_sb4 only) 8 words: 100 MHz real-time at kernel
// start, tower start, tower end, kernel end, the XCC id, and the shader-clock counter at tower start / end.
static int tower_diag_run(azr_engine* h, int n, int warm, std::vector<unsigned long long>& v)
{
    if (!h || !h->net.bf16ctx || !h->weights_set) return AZR_E_STATE;
    Bf16Net* x = bn(h);
    unsigned long long* d = nullptr;
    const size_t words = 8 + 8 * (size_t)(n > 0 ? n : 1);
    HIPCHK(h, hipMalloc((void**)&d, words * sizeof(unsigned long long)));
    HIPCHK(h, hipMemsetAsync(d, 0, words * sizeof(unsigned long long), h->stream));
    for (int i = 0; i < warm; i++) net_bf16_forward(h, h->d.leaf_in, LEAF_STRIDE, n, h->d.net_pi, h->d.net_v, nullptr, h->stream);
    x->diag = d;
    int rc = net_bf16_forward(h, h->d.leaf_in, LEAF_STRIDE, n, h->d.net_pi, h->d.net_v, nullptr, h->stream);
    x->diag = nullptr;
    v.assign(words, 0);
    HIPCHK(h, hipMemcpyAsync(v.data(), d, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    hipFree(d);
    return rc;
}

extern "C" int azr_debug_tower_plan(azr_engine* h, int n, int* boards_per_wg, int* wgs)
{
    if (!h || !h->net.bf16ctx || n < 1) return AZR_E_STATE;
    const int snb = plan_sb(bn(h)->sb_mode, n);
    if (snb) { *boards_per_wg = snb; *wgs = (n + snb - 1) / snb; return AZR_OK; }
    if (bn(h)->sb_mode != 0 && bn(h)->sc_mode != 0 && n <= 128) {   // split-channel tower: 4 workgroups of 64 channels per board pair
        *wgs = ((n + 1) / 2) * 4;
        *boards_per_wg = 2;
        return AZR_OK;
    }
    *wgs = n;   // one board per workgroup (k_tower_bf16<1>)
    *boards_per_wg = 1;
    return AZR_OK;
}

extern "C" int azr_debug_tower_clock(azr_engine* h, int n, int warm, double* ghz_out, double* tower_ms_out)
{
    std::vector<unsigned long long> v;
    int rc = tower_diag_run(h, n, warm, v);
    if (rc) return rc;
    const double cyc = (double)(v[2] - v[0]), rt = (double)(v[3] - v[1]);
    if (ghz_out) *ghz_out = rt > 0 ? cyc / rt * 0.1 : 0.0;
    if (tower_ms_out) *tower_ms_out = rt * 1e-5;  // 100 MHz ticks -> ms
    return AZR_OK;
}

extern "C" int azr_debug_tower_trace(azr_engine* h, int n, int warm, unsigned long long* out8, int cap_wgs, int* wgs_out)
{
    std::vector<unsigned long long> v;
    int rc = tower_diag_run(h, n, warm, v);
    if (rc) return rc;
    int wgs = 0;
    for (int i = 0; i < n && i < cap_wgs; i++) {
        if (v[8 + 8 * (size_t)i] == 0) break;
        for (int k = 0; k < 8; k++) out8[8 * (size_t)i + k] = v[8 + 8 * (size_t)i + k];
        wgs++;
    }
    if (wgs_out) *wgs_out = wgs;
    return AZR_OK;
}
