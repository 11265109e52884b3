// azr_surprise.hpp — policy surprise weighting of a self-play game's training records (KataGo, KataGoMethods.md "Policy Surprise
// Weighting").  This engine's own, off by default (azr_selfplay_set_surprise_weighting, include/azr.h states the rule); the reference
// writes every record once.
//
// A record's surprise is KL(pi || P): the policy that goes into the record against the root node's stored prior.  It is computed where
// the record is staged and kept in a float beside the staging buffer (Dev::stage_kl).  When the game ends its n records share the
// weight n: 1 - share each, and share * n in proportion to their surprise; record r is then written floor(w_r) or ceil(w_r) times by a
// coin of (seed, game seed, r) — the counter-based hash of azr_noise.hpp under domain constants of its own (neither the Dirichlet
// sampler's nor the playout cap's), nothing from the game's minstd_rand0.
//
// fp32 throughout, every operation rounded on its own with the intrinsics of azr_forced.hpp, in the order include/azr.h writes them;
// the logarithm is spelled out here so that tests/surprise_ref.py restates every number bit for bit.
#pragma once
#include "azr_internal.hpp"
#include "azr_noise.hpp"
#include "azr_valuemix.hpp"

namespace azr {

constexpr float PSW_MAX_WEIGHT = 64.0f;   // azr_selfplay_set_surprise_weighting / azr_debug_surprise_weights refuse a larger cap

// natural logarithm: x = 2^e * m with m in (sqrt(1/2), sqrt(2)], ln m = 2 atanh(t) with t = (m - 1) / (m + 1), |t| <= 0.1716, as the
// odd series to t^9 (Horner in t^2).  Arguments below the smallest normal float (zero, subnormals) count as that float.
__device__ __forceinline__ float ln32(float x)
{
    if (x < 1.17549435e-38f) x = 1.17549435e-38f;
    const uint32_t b = __float_as_uint(x);
    int e = (int)(b >> 23) - 127;
    float m = __uint_as_float((b & 0x7FFFFFu) | 0x3F800000u);
    if (m > 1.41421354f) { m = __fmul_rn(m, 0.5f); e += 1; }
    const float t = __fdiv_rn(__fsub_rn(m, 1.0f), __fadd_rn(m, 1.0f));
    const float t2 = __fmul_rn(t, t);
    float p = 0.111111112f;
    p = __fadd_rn(__fmul_rn(p, t2), 0.142857149f);
    p = __fadd_rn(__fmul_rn(p, t2), 0.2f);
    p = __fadd_rn(__fmul_rn(p, t2), 0.333333343f);
    p = __fadd_rn(__fmul_rn(p, t2), 1.0f);
    return __fadd_rn(__fmul_rn((float)e, 0.693147182f), __fmul_rn(__fmul_rn(2.0f, t), p));
}

// KL(pi || P) of one record, lane = move: the terms of the legal moves with pi > 0, summed one after the other in index order
__device__ __forceinline__ float record_surprise(float pi, float P, uint64_t valid)
{
    const uint32_t l = lane_id();
    const bool ok = l < (uint32_t)MOVES && ((valid >> l) & 1ULL) && pi > 0.0f;
    const float term = ok ? __fmul_rn(pi, __fsub_rn(ln32(pi), ln32(P))) : 0.0f;
    float kl = 0.0f;
    for (uint32_t m = 0; m < (uint32_t)MOVES; m++) kl = __fadd_rn(kl, rdlf(term, m));
    return kl > 0.0f ? kl : 0.0f;
}

// S of a game: the n staged surprises summed one after the other in staging order (wave-uniform)
__device__ __forceinline__ float game_surprise_sum(const float* kl, uint32_t n)
{
    float S = 0.0f;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t r = base + lane_id();
        const float v = r < n ? kl[r] : 0.0f;
        const uint32_t cnt = n - base < 64u ? n - base : 64u;
        for (uint32_t j = 0; j < cnt; j++) S = __fadd_rn(S, rdlf(v, j));
    }
    return S;
}

// w_r of a record with surprise `kl` in a game of n records whose surprises sum to S
__device__ __forceinline__ float record_weight(float kl, float S, uint32_t n, float share, float max_weight)
{
    if (!(S > 0.0f)) return 1.0f;
    const float w = __fadd_rn(__fsub_rn(1.0f, share), __fmul_rn(__fmul_rn(share, (float)n), __fdiv_rn(kl, S)));
    return w < max_weight ? w : max_weight;
}

// c_r: floor(w) copies, one more if the record's coin falls below the fraction
__device__ __forceinline__ uint32_t record_copies(float w, uint32_t seed, uint32_t game_seed, uint32_t r)
{
    const uint32_t base = (uint32_t)w;
    const uint32_t thr = (uint32_t)__fmul_rn(__fsub_rn(w, (float)base), 16777216.0f);
    uint32_t k = noise_mix(seed + 0x165667B1u);
    k = noise_mix(k ^ game_seed);
    k = noise_mix((k ^ r) + 0xD3A2646Cu);
    return base + ((k >> 8) < thr ? 1u : 0u);
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m);
    return v;
}

// flush_samples under surprise weighting: the finished game's n staged records (surprises in E.stage_kl), record r written c_r times
// in a row, in staging order, into ONE ring reservation of C = sum c_r records.  Returns C; copies past the ring's end are counted in
// `dropped`.  Lane r of a 64-record chunk computes c_r; the copies are then written record by record in flush_samples' packing
// (record_byte), every copy of a record with the same z — under QMIX the blended one (azr_valuemix.hpp).
template <bool QMIX = false>
__device__ __forceinline__ unsigned long long flush_samples_weighted(const Dev& E, int g, uint32_t n, int status, uint32_t game_seed,
                                                                     unsigned long long& dropped)
{
    if (n == 0) return 0;
    const float* kl = E.stage_kl + (size_t)g * E.SCAP;
    const float S = game_surprise_sum(kl, n);
    unsigned long long C = 0;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t r = base + lane_id();
        C += wave_sum_u32(r < n ? record_copies(record_weight(kl[r], S, n, E.psw_share, E.psw_max), E.psw_seed, game_seed, r) : 0u);
    }
    if (C == 0) return 0;
    unsigned long long slot = 0;
    if (lane_id() == 0) slot = atomicAdd(E.ring_count, C);
    slot = rfl64(slot);
    const uint8_t* st = E.stage + (size_t)g * E.SCAP * STAGE_BYTES;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t rl = base + lane_id();
        const uint32_t cl = rl < n ? record_copies(record_weight(kl[rl], S, n, E.psw_share, E.psw_max), E.psw_seed, game_seed, rl) : 0u;
        const uint32_t cnt = n - base < 64u ? n - base : 64u;
        for (uint32_t j = 0; j < cnt; j++) {
            const uint32_t copies = rdl(cl, j);
            if (copies == 0) continue;
            const uint8_t* src = st + (size_t)(base + j) * STAGE_BYTES;
            const uint32_t player = rfl((uint32_t)src[260]);
            const uint32_t zb = record_z_bits<QMIX>(E, g, base + j, player, status);
            // this lane's bytes of the 265-byte record (byte i * 64 + lane), read once for all the copies
            uint8_t b[5];
#pragma unroll
            for (uint32_t i = 0; i < 5; i++) {
                const uint32_t q = i * 64u + lane_id();
                b[i] = q < AZR_RECORD_BYTES ? record_byte(src, player, zb, q) : (uint8_t)0;
            }
            for (uint32_t cpy = 0; cpy < copies; cpy++, slot++) {
                if (slot >= E.ring_cap) { dropped += 1; continue; }
                uint8_t* dst = E.ring + (size_t)slot * AZR_RECORD_BYTES;
#pragma unroll
                for (uint32_t i = 0; i < 5; i++) {
                    const uint32_t q = i * 64u + lane_id();
                    if (q < AZR_RECORD_BYTES) dst[q] = b[i];
                }
            }
        }
    }
    return C;
}

}  // namespace azr
