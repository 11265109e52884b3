// azr_valuemix.hpp — blending the search's root value into the z of a self-play game's training records (Lc0's q_ratio; z/q averaging
// in Oracle's "Lessons from AlphaZero").  This engine's own, off by default (azr_selfplay_set_value_mix, include/azr.h states the rule);
// the reference writes the bare game outcome.
//
// The root value q of a recorded decision is the visit-weighted mean of the root node's Q over the legal moves the search completed a
// visit of, from the root mover's perspective — the record's.  It is computed where the record is staged and kept in a float beside the
// staging buffer (Dev::stage_q, NaN = the root had no completed visit).  When the game ends, the outcome z of every record becomes
// z' = (1 - q_share) * z + q_share * q.  Nothing else in the record, and nothing in the search, depends on it.
//
// fp32 throughout, every operation rounded on its own with the intrinsics of azr_forced.hpp, in the order include/azr.h writes them, so
// that tests/value_mix_ref.py restates every number bit for bit.  Also here, once for both flush paths: a record's z and the 265-byte
// packing of a staged record.
#pragma once
#include "azr_internal.hpp"

namespace azr {

// q of a root, lane = move: N = the completed visits (the unpruned count), Q = the mean values, valid = the legal moves.  Sum(N * Q) and
// Sum(N) over the legal moves with N > 0, summed one after the other in index order; has_q = Sum(N) > 0, q = 0 without it (wave-uniform).
__device__ __forceinline__ float root_value(uint32_t N, float Q, uint64_t valid, bool& has_q)
{
    const uint32_t l = lane_id();
    const bool ok = l < (uint32_t)MOVES && ((valid >> l) & 1ULL) && N > 0u;
    const float fn = ok ? (float)N : 0.0f;
    const float term = ok ? __fmul_rn(fn, Q) : 0.0f;
    float num = 0.0f, den = 0.0f;   // a move that does not count adds +0.0f, which leaves a sum that started at +0.0f as it is
    for (uint32_t m = 0; m < (uint32_t)MOVES; m++) {
        num = __fadd_rn(num, rdlf(term, m));
        den = __fadd_rn(den, rdlf(fn, m));
    }
    has_q = den > 0.0f;
    if (!has_q) return 0.0f;
    float q = __fdiv_rn(num, den);
    q = q < -1.0f ? -1.0f : q;
    return q > 1.0f ? 1.0f : q;
}

// z' of a record with the outcome z and the root value q; a = 1 - q_share
__device__ __forceinline__ float blend_z(float z, float q, bool has_q, float a, float q_share)
{
    if (!has_q) return z;
    float b = __fadd_rn(__fmul_rn(a, z), __fmul_rn(q_share, q));
    b = b < -1.0f ? -1.0f : b;
    return b > 1.0f ? 1.0f : b;
}

// The value of staged record r of slot g whose game ended with `status`, as its four record bytes: NNTrainDataStorage::updateValues
// (alphazero_nn_data.cpp:51-65) for the record's player — under QMIX blended with the root value staged beside the record.
template <bool QMIX>
__device__ __forceinline__ uint32_t record_z_bits(const Dev& E, int g, uint32_t r, uint32_t player, int status)
{
    float z = status == ST_DRAW ? 0.0f : ((int)player == status ? 1.0f : -1.0f);
    if (QMIX) {
        const float q = rdlf(E.stage_q[(size_t)g * E.SCAP + r], 0);
        z = blend_z(z, q, q == q, __fsub_rn(1.0f, E.q_share), E.q_share);
    }
    return __float_as_uint(z);
}

// Byte j < 265 of the on-disk record (alphazero_nn_data.cpp:123-130) of the staged record at `src` (in88 @0 | pi[43] @88 | player @260):
// player | in88 | z | pi
__device__ __forceinline__ uint8_t record_byte(const uint8_t* src, uint32_t player, uint32_t zb, uint32_t j)
{
    uint8_t b;
    if (j == 0) b = (uint8_t)player;
    else if (j < 89) b = src[j - 1];
    else if (j < 93) b = (uint8_t)(zb >> (8 * (j - 89)));
    else b = src[88 + (j - 93)];
    return b;
}

}  // namespace azr
