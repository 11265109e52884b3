// azr_tower_common.hpp — what the multi-board LDS-resident towers (k_tower_sb, k_tower_sc, k_tower_fx) share beyond
// azr_bf16_common.hpp: the table region of their LDS maps, the launch prologue (input staging, zero rows, stem features; the row
// tables themselves: build_row_tables, azr_rowclass.hpp) and the 16-bit layer epilogue.  k_tower_bf16<1> (azr_net_bf16.hip) takes
// nothing from here: it is the independently written kernel the others are compared with, bit for bit.
#pragma once
#include "azr_bf16_common.hpp"
#include "azr_rowclass.hpp"

namespace azr {

// The table region of a tower's LDS map, BASE bytes into it, for NB boards in ZR rows (16-byte aligned at both ends if BASE is)
template <int NB, int ZR, int BASE>
struct TowerTables {
    static constexpr int IN88_OFF = BASE;                       // NB x 96 B NNInputData images
    static constexpr int ROWOF_OFF = IN88_OFF + NB * 96;        // u8 [ZR]: cell (board * 42 + pos) -> row
    static constexpr int TAPROW_OFF = ROWOF_OFF + ZR;           // u8 [10][ZR]: source row of (tap, row); tap 9 = all zero row
    static constexpr int ROWCELL_OFF = TAPROW_OFF + 10 * ZR;    // u16 [ZR]: row -> y | x << 4 | board << 8, 0xffff = pad row
    static constexpr int END = (ROWCELL_OFF + 2 * ZR + 15) / 16 * 16;
    static_assert(TAPROW_OFF % 4 == 0 && ROWCELL_OFF % 2 == 0, "alignment");
};

// ---- launch prologue.  No barrier in these three: the callers' barriers stand where they stood.  A kernel writes a piece out instead of
// calling it where the call changes its instruction text from its first MFMA on (profiles/tower_common_isa.txt: k_tower_sc's input
// staging; k_tower_fx's table loops, which still apply the rules of azr_rowclass.hpp).
// the NNInputData images of boards board0 .. board0 + NB - 1 (of n; a missing board reads as zeros), 96 bytes each
template <int NB, int THREADS>
__device__ __forceinline__ void stage_inputs(uint8_t* in_l, const uint8_t* in88, int in_stride, int board0, int n, const int* slot_map)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < NB * 96; i += THREADS) {
        const int b = i / 96, o = i % 96;
        const int slot = (board0 + b < n) ? (slot_map ? slot_map[board0 + b] : board0 + b) : 0;
        in_l[i] = (board0 + b < n && o < 88) ? in88[(size_t)slot * in_stride + o] : (uint8_t)0;
    }
}
// the zero rows of a tower's N activation images (the source of pad rows, out-of-board taps and tap 9)
template <int THREADS, class... Row>
__device__ __forceinline__ void clear_zero_rows(Row*... row)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < ROWB / 4; i += THREADS) ((reinterpret_cast<uint32_t*>(row)[i] = 0), ...);
}
// stem features as feat[ZR + 1][16] (row ZR = zero row; planes 13..15 are zero) in the tower's format: cvt(v) of the plane value v
template <int ZR, int THREADS, class T, class Cvt>
__device__ __forceinline__ void stem_features(const uint8_t* in_l, const uint16_t* rowcell, T* feat, Cvt cvt)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < (ZR + 1) * 16; i += THREADS) {
        const int r = i >> 4, ch = i & 15;
        float v = 0.0f;
        const int ci = r < ZR ? rowcell[r] : 0xffff;
        if (ci != 0xffff) v = plane_value(in_l + (ci >> 8) * 96, (ci & 15) * 6 + ((ci >> 4) & 15), ch);
        feat[i] = cvt(v);
    }
}

__device__ __forceinline__ s16x8 lds16(const uint8_t* p) { return *reinterpret_cast<const s16x8*>(p); }

// Layer epilogue of the 16-bit towers for 4 consecutive channels of one board cell: folded BN (fp32 fma), optional shortcut add (the
// packed block input), ReLU, round-to-nearest-even.  Packed forms: v_pk_fma_f32 / v_pk_add_f32 / v_cvt_pk_bf16_f32 / v_pk_max_i16 —
// ReLU is applied to the ROUNDED value as a signed 16-bit max with 0 (rounding is monotonic and odd, so relu(rne(v)) == rne(relu(v));
// -0 becomes +0 like `v > 0 ? v : 0`).
template <bool SHORTCUT, bool F16>
__device__ __forceinline__ uint2 bn_relu_pack(const f32x4& acc, const float4& s, const float4& h, const uint2& x)
{
    // (the two instantiations are kept apart on purpose: merged by the optimiser, the common fma of all 44 tiles of k_tower_sb<4> is
    //  hoisted above the parity branch and 176 intermediate values have to be parked)
    f32x4 t = acc;
    if (SHORTCUT) asm volatile("; epilogue with shortcut" : "+v"(t));
    else asm volatile("; epilogue" : "+v"(t));
    f32x2 lo = __builtin_elementwise_fma(f32x2{t[0], t[1]}, f32x2{s.x, s.y}, f32x2{h.x, h.y});
    f32x2 hi = __builtin_elementwise_fma(f32x2{t[2], t[3]}, f32x2{s.z, s.w}, f32x2{h.z, h.w});
    if (SHORTCUT) {
        lo += f32x2{El<F16>::lo_of(x.x), El<F16>::hi_of(x.x)};
        hi += f32x2{El<F16>::lo_of(x.y), El<F16>::hi_of(x.y)};
    }
    return uint2{El<F16>::pack_relu(lo), El<F16>::pack_relu(hi)};
}

}  // namespace azr
