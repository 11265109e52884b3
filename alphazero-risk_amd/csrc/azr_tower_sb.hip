// azr_tower_sb.hip — k_tower_sb<NB>: the whole policy/value net (python/src/build_graph.py:63-90) for NB = 2, 3 or 4 boards per
// workgroup with ONE LDS activation image (gfx950).
//
// Why a second tower kernel.  k_tower_bf16 (azr_net_bf16.hip) keeps two ping-pong activation images in LDS, which caps a
// workgroup at 3 boards (M = 128 GEMM rows), and its 8 waves x 32 channels read every activation fragment for 2 MFMAs only.
// Here a workgroup owns up to 4 boards (168 cells, 11 MFMA row tiles) in a SINGLE LDS image:
//   * a layer's whole output lives in accumulator registers until the layer's last k-step (it always did); the image is
//     overwritten in place between two barriers (all waves done reading | epilogue stores | all stores visible);
//   * the residual input of a block — the values this wave itself stored two layers earlier — stays packed (bf16) in
//     registers instead of in a second image (at 4 boards 176 accumulators + 88 residual registers + ring + fragments fill
//     the 512-register file to the last one: the residual registers are updated in place, see the layer epilogue);
//   * 4 waves (one per SIMD, up to 512 registers each) split the 256 output channels, 64 (four 16-wide tiles) each, so an
//     activation fragment read from LDS feeds 4 MFMAs: LDS fragment traffic per MFMA is half that of the 8-wave tiles;
//   * per k-step a wave issues, tile by tile, [4 MFMAs | 1 ds_read_b128 of that tile's NEXT k-step fragment]; the 4 buffer
//     loads that refill the weight-ring slot freed by the previous k-step, and the next tap's row-table lookups, are dealt
//     out over the k-step, one per MFMA gap (ring of 4 slots, 3 k-steps ahead, never drained; the packed stream of all
//     layers is contiguous, exactly as for k_tower_bf16 — both kernels read the same packed weights);
//   * the layer loop is rolled (conv1 and conv2 of a block share the code; only the epilogue looks at the parity) and a
//     layer's 72 k-steps are fully unrolled with compile-time skip masks: ~40 KB of straight-line code, inside the
//     64 KB instruction cache;
//   * a layer's folded BN scale / shift reach the epilogue through LDS (2 registers per lane over the k-steps, not 32).
// Row order (border classes with the corners in the column classes, azr_rowclass.hpp): 18 of 99 / 12 of 72 / 9 of 54
// (tile, tap) pairs are entirely out of board and are skipped.
// Arithmetic is the k_tower_bf16 arithmetic — same k order, same fp32 epilogue, same RNE points — so results are
// bit-identical across tile shapes (tests/test_gpu_net.py checks it).
// The launch prologue, the table region of the LDS map and the layer epilogue are the ones of azr_tower_common.hpp.
#include <stdlib.h>
#include <string.h>

#include "azr_internal.hpp"
#include "azr_tower_common.hpp"

using namespace azr;

namespace {
constexpr int NT = 4;                  // 16-channel column tiles per wave (4 waves x 64 channels)
constexpr int WAVES = 4, THREADS = 256;

// Geometry of a workgroup of NB boards (NB = 4: the product tile; NB = 2: the tile for 257..512 boards per launch).
template <int NB_>
struct SB {
    static constexpr int NB = NB_;                       // boards per workgroup
    static constexpr int ROWS = 42 * NB;                 // board cells
    static constexpr int MT = (ROWS + 15) / 16;          // 16-row MFMA tiles: 11 (8 pad rows) / 6 (12 pad rows)
    static constexpr int ZR = MT * 16;                   // index of the shared zero row
    static constexpr int RING = 4;                         // weight ring depth in k-steps (72 = 0 mod RING)
    // LDS map
    static constexpr int BUF = (ZR + 1) * ROWB;                 // the activation image incl. its zero row     96 288 B at NB = 4
    static constexpr int FEAT_OFF = BUF;                        // stem features [(ZR + 1)][16 bf16]             5 664 B
    static constexpr int HEAD_OFF = FEAT_OFF + (ZR + 1) * FROWB;  // heads scratch: NB x (128 + 256 + 64) floats 7 168 B
    using TAB = TowerTables<NB, ZR, HEAD_OFF + NB * 448 * 4>;   // NNInputData images and row tables
    static constexpr int FOLD_OFF = TAB::END;                   // float [2][256]: the current layer's folded BN scale | shift
    static constexpr int LDS_BYTES = FOLD_OFF + 2 * NF * 4;
    static_assert(NB >= 2 && NB <= 4, "tile shapes");
    static_assert(72 % RING == 0 && RING <= MAX_RING, "ring depth");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
    static_assert(BUF % 16 == 0 && FEAT_OFF % 16 == 0 && HEAD_OFF % 16 == 0 && FOLD_OFF % 16 == 0, "alignment");
    static_assert(3 * NF * 4 <= (ZR + 1) * FROWB, "the heads stage 3 x 256 floats in the stem feature image");
};

// s_waitcnt lgkmcnt(N) alone (vmcnt / expcnt untouched)
template <int N>
__device__ __forceinline__ void wait_lgkm()
{
    if constexpr (N >= 0 && N <= 14) __builtin_amdgcn_s_waitcnt(0xC07F | (N << 8));
}

// One tap (8 k-steps of 32 input channels) of a 3x3 conv layer for the 11 row tiles x 4 column tiles of a wave.  Everything
// that depends on the tap — which tiles run (skip masks), ring slots, wait counts — is a compile-time constant.
//
// Issue order.  A lone wave issues one instruction per ~4 cycles and an MFMA occupies the issue port for 8 of its 16 cycles:
// whatever else sits in one MFMA gap beyond ~8 cycles delays the matrix pipe.  So the non-MFMA work of a k-step is dealt out
// one piece per gap instead of in bursts:
//   k-step start:  one counted vmcnt wait for all four weight fragments of this k-step (the loads of the two k-steps in
//                  flight behind them stay outstanding)
//   per tile:      M0 | [one refill load] | M1 | [wait for the NEXT tile's fragment] | M2 | M3 | re-read of this tile's
//                  fragment for the next k-step
// The compiler's own waitcnt insertion still runs afterwards and stays the safety net: an explicit wait only moves a wait
// to an earlier, cheaper place.
template <int NB, int TAP, bool F16>
__device__ __forceinline__ void conv_tap(const uint8_t* bufX, const uint8_t* tr_c, uint32_t g16, const __amdgpu_buffer_rsrc_t wsrc,
                                         uint32_t loff, uint32_t& wk, u32x4 (&bq)[SB<NB>::RING][NT], f32x4 (&acc)[SB<NB>::MT][NT],
                                         s16x8 (&a)[SB<NB>::MT], uint32_t (&ap)[SB<NB>::MT])
{
    constexpr int MT = SB<NB>::MT, ZR = SB<NB>::ZR, RING = SB<NB>::RING;
    constexpr uint32_t sk = skip_mask<NB>(TAP), skn = skip_mask<NB>(TAP + 1);
    constexpr int active = MT - __builtin_popcount(sk & ((1u << MT) - 1u));   // tiles that run this tap
    uint32_t np[MT];
#pragma unroll
    for (int ks = 0; ks < KS_PER_TAP; ks++) {
        const int gk = TAP * KS_PER_TAP + ks;                       // k-step inside the layer (72 = 0 mod RING)
        const int cur = gk % RING, ref = (gk + RING - 1) % RING;    // ring slot in use / slot freed by the previous k-step
        {   // vmcnt((RING - 2) * NT): this k-step's four fragments have landed, the younger k-steps stay in flight
            constexpr int VM = (RING - 2) * NT;
            __builtin_amdgcn_s_waitcnt(0x0F70 | (VM & 15) | ((VM >> 4) << 14));   // lgkmcnt / expcnt untouched
        }
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            if (!((sk >> mt) & 1u)) {
                const int j = __builtin_popcount(~sk & ((1u << mt) - 1u));   // index among the active tiles
                acc[mt][0] = El<F16>::mfma(bq[cur][0], a[mt], acc[mt][0]);
                // refill of the slot the previous k-step freed, RING - 1 k-steps ahead: one of its 4 loads after the first
                // MFMA of 4 tiles spread over the k-step (also across layer boundaries)
#pragma unroll
                for (int nt = 0; nt < NT; nt++)
                    if (j == ((nt + 1) * active) / NT - 1)
                        bq[ref][nt] = __builtin_amdgcn_raw_buffer_load_b128(wsrc, loff + nt * 1024, (int)(wk + (RING - 1) * KBYTES), 0);
                __builtin_amdgcn_sched_barrier(0);
                acc[mt][1] = El<F16>::mfma(bq[cur][1], a[mt], acc[mt][1]);
                wait_lgkm<active - 2>();                            // the next tile's fragment was requested `active - 1` reads ago
                __builtin_amdgcn_sched_barrier(0);
                acc[mt][2] = El<F16>::mfma(bq[cur][2], a[mt], acc[mt][2]);
                acc[mt][3] = El<F16>::mfma(bq[cur][3], a[mt], acc[mt][3]);
                if (ks < KS_PER_TAP - 1) a[mt] = lds16(bufX + ap[mt] + (ks + 1) * 64);
            }
            // the next tap's source rows, dealt out like everything else: one table byte per tile slot two k-steps before
            // the tap ends, its address arithmetic one k-step later (as a burst in front of a k-step they cost ~3 % of a layer)
            if (ks == KS_PER_TAP - 3) { if (!((skn >> mt) & 1u)) np[mt] = (uint32_t)tr_c[(TAP + 1) * ZR + mt * 16]; }
            if (ks == KS_PER_TAP - 2) { if (!((skn >> mt) & 1u)) np[mt] = np[mt] * ROWB + g16; }
            if (ks == KS_PER_TAP - 1) { if (!((skn >> mt) & 1u)) a[mt] = lds16(bufX + np[mt]); }
            __builtin_amdgcn_sched_barrier(0);
        }
        wk += (uint32_t)KBYTES;
    }
#pragma unroll
    for (int mt = 0; mt < MT; mt++) ap[mt] = np[mt];
}

template <int NB, bool F16>
__global__ __launch_bounds__(THREADS, 1) void k_tower_sb(const uint8_t* __restrict__ in88, int in_stride, int n,
                                                          const uint16_t* __restrict__ stem_wp, const uint16_t* __restrict__ tower_wp,
                                                          const float* __restrict__ fold, int blocks, const float* __restrict__ hp,
                                                          float* __restrict__ pi_out, float* __restrict__ v_out,
                                                          unsigned long long* __restrict__ diag, const int* __restrict__ slot_map)
{
    using G = SB<NB>;
    constexpr int ROWS = G::ROWS, MT = G::MT, ZR = G::ZR, RING = G::RING;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t* bufX = lds;
    uint8_t* bufF = lds + G::FEAT_OFF;
    uint8_t* in_l = lds + G::TAB::IN88_OFF;
    uint8_t* rowof = lds + G::TAB::ROWOF_OFF;
    uint8_t* taprow = lds + G::TAB::TAPROW_OFF;
    uint16_t* rowcell = reinterpret_cast<uint16_t*>(lds + G::TAB::ROWCELL_OFF);
    float* foldl = reinterpret_cast<float*>(lds + G::FOLD_OFF);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;        // MFMA fragment coordinates: board cell (column) c of a tile, k-group g
    const int board0 = blockIdx.x * NB;
    // diagnostics (azr_debug_tower_clock / azr_debug_tower_trace; `diag` is null in every product launch): workgroup 0's
    // shader-clock / real-time stamps around the tower, and per workgroup 8 words from diag[8 + 8 * blockIdx]: real-time
    // at kernel start, tower start, tower end, kernel end, and the XCC the workgroup ran on
    if (diag && blockIdx.x == 0 && tid == 0) { diag[0] = __builtin_amdgcn_s_memtime(); diag[1] = __builtin_amdgcn_s_memrealtime(); }
    if (diag && tid == 0) {
        diag[8 + 8 * (size_t)blockIdx.x] = __builtin_amdgcn_s_memrealtime();
        diag[8 + 8 * (size_t)blockIdx.x + 4] = __builtin_amdgcn_s_getreg((20 /*HW_REG_XCC_ID*/) | (0 << 6) | (3 << 11)) & 15u;
    }

    // ---- weight ring: the first RING - 1 k-steps of layer 0 fly while the tables and the stem are built
    const __amdgpu_buffer_rsrc_t wsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(tower_wp), (short)0, 0x7fffffff, 0x00020000);
    const uint32_t loff = (uint32_t)((wave * NT) * 64 + lane) * 16u;   // this lane's fragment bytes inside a k-step block
    uint32_t wk = 0;                                                     // byte offset of the current k-step (wave-uniform)
    u32x4 bq[RING][NT];
#pragma unroll
    for (int ks = 0; ks < RING - 1; ks++)   // (slot RING - 1 is filled during k-step 0, and so on: the refill of a slot is
                                            //  issued during the k-step after the one that used it)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) bq[ks][nt] = __builtin_amdgcn_raw_buffer_load_b128(wsrc, loff + nt * 1024, ks * (int)KBYTES, 0);

    // ---- stage the NNInputData images, build the row tables and the stem features (bufF: row ZR = zero row)
    stage_inputs<NB, THREADS>(in_l, in88, in_stride, board0, n, slot_map);
    clear_zero_rows<THREADS>(bufX + ZR * ROWB);
    build_row_tables<NB, THREADS, 10>(rowof, taprow, rowcell);
    stem_features<ZR, THREADS>(in_l, rowcell, reinterpret_cast<uint16_t*>(bufF), [](float v) { return El<F16>::rne(v); });
    __syncthreads();

    f32x4 acc[MT][NT];
    // the block input of this wave's (cell, 4-channel) elements, packed bf16 = the residual operand
    uint2 res[MT][NT];
    const uint32_t eoff = (uint32_t)(c * ROWB + (wave * 64 + g * 4) * 2);   // epilogue store address of tile 0 / column tile 0

    // ---- stem: 3x3 conv 13 -> 256, two taps per 32-deep k-step (tap = 2*ks + (g >> 1), channels (g & 1)*8 ..), weights as
    //      the MFMA "A" operand: D[channel][cell], a lane ends up with 4 consecutive channels of one board cell
    {
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int nt = 0; nt < NT; nt++) acc[mt][nt] = f32x4{0, 0, 0, 0};
        const s16x8* wp = reinterpret_cast<const s16x8*>(stem_wp) + (size_t)(wave * NT) * 64 + lane;
#pragma unroll
        for (int ks = 0; ks < STEM_KS; ks++) {
            const int tap = 2 * ks + (g >> 1);   // 0..9; tap 9 (second half of the last k-step) is the zero row
            s16x8 b[NT];
#pragma unroll
            for (int nt = 0; nt < NT; nt++) b[nt] = wp[(size_t)ks * FRAGS_PER_KSTEP * 64 + nt * 64];
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                const int row = taprow[tap * ZR + mt * 16 + c];
                const s16x8 av = lds16(bufF + row * FROWB + (g & 1) * 16);
#pragma unroll
                for (int nt = 0; nt < NT; nt++)
                    acc[mt][nt] = El<F16>::mfma(b[nt], av, acc[mt][nt]);
            }
        }
        // conv_bn over the board ROW (build_graph.py:68 axis=1) + ReLU
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            const int ci = rowcell[mt * 16 + c];
            const int y = ci == 0xffff ? 0 : (ci & 15);
            const float sc = fold[y], sh = fold[7 + y];
#pragma unroll
            for (int nt = 0; nt < NT; nt++) {
                const uint2 o = bn_relu_pack<false, F16>(acc[mt][nt], float4{sc, sc, sc, sc}, float4{sh, sh, sh, sh}, uint2{0, 0});
                res[mt][nt] = o;
                if (c < pad_from<NB>(mt)) *reinterpret_cast<uint2*>(bufX + eoff + mt * 16 * ROWB + nt * 32) = o;
            }
        }
    }
    __syncthreads();

    if (diag && tid == 0) { diag[8 + 8 * (size_t)blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime(); diag[8 + 8 * (size_t)blockIdx.x + 5] = __builtin_amdgcn_s_memtime(); }
    // ---- residual tower: 2B conv layers, activations resident in the one LDS image
    const uint8_t* tr_c = taprow + c;           // this lane's column of the (tap, row) -> source-row table
    const uint32_t g16 = (uint32_t)g * 16u;
    const int layers = 2 * blocks;
    for (int L = 0; L < layers; L++) {
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int nt = 0; nt < NT; nt++) acc[mt][nt] = f32x4{0, 0, 0, 0};
        const float2 fnext = *reinterpret_cast<const float2*>(fold + 14 + (size_t)L * 2 * NF + 2 * tid);   // (see the epilogue)
        uint32_t ap[MT];        // LDS byte address of this lane's fragment of tile mt at k-step 0 of the current tap
        s16x8 a[MT];            // ... and the fragment of the k-step about to run
        {
            const uint32_t sk0 = skip_mask<NB>(0);
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                ap[mt] = (uint32_t)tr_c[mt * 16] * ROWB + g16;
                if (!((sk0 >> mt) & 1u)) a[mt] = lds16(bufX + ap[mt]);
            }
        }
        conv_tap<NB, 0, F16>(bufX, tr_c, g16, wsrc, loff, wk, bq, acc, a, ap);
        conv_tap<NB, 1, F16>(bufX, tr_c, g16, wsrc, loff, wk, bq, acc, a, ap);
        conv_tap<NB, 2, F16>(bufX, tr_c, g16, wsrc, loff, wk, bq, acc, a, ap);
        conv_tap<NB, 3, F16>(bufX, tr_c, g16, wsrc, loff, wk, bq, acc, a, ap);
        conv_tap<NB, 4, F16>(bufX, tr_c, g16, wsrc, loff, wk, bq, acc, a, ap);
        conv_tap<NB, 5, F16>(bufX, tr_c, g16, wsrc, loff, wk, bq, acc, a, ap);
        conv_tap<NB, 6, F16>(bufX, tr_c, g16, wsrc, loff, wk, bq, acc, a, ap);
        conv_tap<NB, 7, F16>(bufX, tr_c, g16, wsrc, loff, wk, bq, acc, a, ap);
        conv_tap<NB, 8, F16>(bufX, tr_c, g16, wsrc, loff, wk, bq, acc, a, ap);
        // this layer's folded BN scale / shift go through LDS: 2 registers per lane over the k-steps instead of 32 (which the
        // register allocator parked in scratch), written before the barrier, read back 16 bytes at a time after it
        *reinterpret_cast<float2*>(foldl + 2 * tid) = fnext;
        __syncthreads();        // every wave has read the image for the last time
        float4 sc[NT], sh[NT];
#pragma unroll
        for (int nt = 0; nt < NT; nt++) {
            sc[nt] = *reinterpret_cast<const float4*>(foldl + wave * 64 + g * 4 + nt * 16);
            sh[nt] = *reinterpret_cast<const float4*>(foldl + NF + wave * 64 + g * 4 + nt * 16);
        }
        // Two conditions in a row, not if / else, and the second one opaque to the optimiser: as one diamond the control flow is
        // restructured with the new residual values merged against "undefined" while the old ones are still live, the two sets
        // cannot share registers, and 88 registers get copied out and back in every layer.  This way `res` is updated in place
        // (and only so do 88 residual registers fit at 4 boards: after a compiler update check -Rpass-analysis=kernel-resource-usage
        // for zero scratch and zero spills in all six instantiations).
        int even = ~L & 1;
        asm volatile("" : "+s"(even));
        if (L & 1) {    // second conv of a block: + shortcut (the block's input, kept packed in registers), and this
                        // output is the next block's input
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int nt = 0; nt < NT; nt++) {
                    const uint2 o = bn_relu_pack<true, F16>(acc[mt][nt], sc[nt], sh[nt], res[mt][nt]);
                    res[mt][nt] = o;
                    if (c < pad_from<NB>(mt)) *reinterpret_cast<uint2*>(bufX + eoff + mt * 16 * ROWB + nt * 32) = o;
                }
        }
        if (even) {
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int nt = 0; nt < NT; nt++) {
                    const uint2 o = bn_relu_pack<false, F16>(acc[mt][nt], sc[nt], sh[nt], uint2{0, 0});
                    if (c < pad_from<NB>(mt)) *reinterpret_cast<uint2*>(bufX + eoff + mt * 16 * ROWB + nt * 32) = o;
                }
        }
        __syncthreads();        // the new image is complete
    }

    if (diag && blockIdx.x == 0 && tid == 0) { diag[2] = __builtin_amdgcn_s_memtime(); diag[3] = __builtin_amdgcn_s_memrealtime(); }
    if (diag && tid == 0) { diag[8 + 8 * (size_t)blockIdx.x + 2] = __builtin_amdgcn_s_memrealtime(); diag[8 + 8 * (size_t)blockIdx.x + 6] = __builtin_amdgcn_s_memtime(); }
    // ---- both heads; the stem's feature image is free by now and holds the 1x1-conv weight columns
    fused_heads<NB, THREADS>(tid, hp, reinterpret_cast<float*>(bufF), reinterpret_cast<float*>(lds + G::HEAD_OFF), rowof, ImageAct<F16>{bufX},
                             board0, n, slot_map, pi_out, v_out);
    if (diag && tid == 0) diag[8 + 8 * (size_t)blockIdx.x + 3] = __builtin_amdgcn_s_memrealtime();
}
}  // namespace

namespace azr {

// the one <NB, F16> ladder: f(tile shape) for the handle's element type and nb = 2, 3 or 4 boards per workgroup
template <int NB, bool F16> struct Shape { static constexpr int nb = NB; static constexpr bool f16 = F16; };
template <class Fn>
static int sb_dispatch(azr_engine* h, int nb, Fn f)
{
    if (bf16net(h)->f16) return nb == 4 ? f(Shape<4, true>{}) : nb == 3 ? f(Shape<3, true>{}) : f(Shape<2, true>{});
    return nb == 4 ? f(Shape<4, false>{}) : nb == 3 ? f(Shape<3, false>{}) : f(Shape<2, false>{});
}

int tower_sb_init(azr_engine* h)
{
    for (int nb = 4; nb >= 2; nb--) {
        const int rc = sb_dispatch(h, nb, [&](auto s) -> int {
            constexpr int NB = decltype(s)::nb;
            constexpr bool F16 = decltype(s)::f16;
            HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(k_tower_sb<NB, F16>), hipFuncAttributeMaxDynamicSharedMemorySize, SB<NB>::LDS_BYTES));
            return AZR_OK;
        });
        if (rc) return rc;
    }
    return AZR_OK;
}

// `wgs` workgroups of nb (2, 3 or 4) boards: boards [0, n) of the launch (the last workgroup may be partly filled)
int tower_sb_launch(azr_engine* h, int nb, int wgs, const uint8_t* d_in88, int in_stride, int n, float* d_pi, float* d_v, const int* d_map, hipStream_t st)
{
    if (nb < 2 || nb > 4 || wgs < 1 || (long long)wgs * nb < n) { h->err = "tower_sb_launch: bad tiling"; return AZR_E_INVALID_ARGUMENT; }
    Bf16Net* x = bf16net(h);
    sb_dispatch(h, nb, [&](auto s) {
        constexpr int NB = decltype(s)::nb;
        constexpr bool F16 = decltype(s)::f16;
        hipLaunchKernelGGL((k_tower_sb<NB, F16>), dim3(wgs), dim3(THREADS), SB<NB>::LDS_BYTES, st, d_in88, in_stride, n, x->stem_wp, x->tower_wp,
                           F16 ? (const float*)x->fold16 : net_fold(h), h->net.blocks, net_head_params(h), d_pi, d_v, x->diag, d_map);
        return 0;
    });
    HIPCHK(h, hipGetLastError());
    return AZR_OK;
}

}  // namespace azr
