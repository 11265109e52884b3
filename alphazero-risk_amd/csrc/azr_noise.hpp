// azr_noise.hpp — Dirichlet(alpha) root noise, one wavefront per root (gfx950, wave64): lane m < 43 draws g_m ~ Gamma(alpha, 1) for
// the legal move m, eta_m = g_m / sum over the legal moves; illegal lanes are 0.  This engine's own: the reference mixes the
// constant DIR_NOISE_EPSI * DIR_NOISE_VALUE into every prior (alphazero_mcts.cpp:81) and samples nothing.
//
// The draw is a function of (noise_seed, game seed, decision, move, alpha) alone — a counter-based generator, no state: lane m's
// stream is keyed by a 32-bit integer hash of the four integers, its i-th uniform is the hash of key + i * golden ratio.  Nothing is
// taken from the game's minstd_rand0, so dice, deals and move sampling stay on the reference's stream.
//
// Gamma: Marsaglia-Tsang ("A simple method for generating gamma variables", 2000) at shape a = alpha (alpha >= 1) or alpha + 1 with
// the U^(1/alpha) boost (alpha < 1), normals by Box-Muller, kept in LOG space: lg = log d + log v [+ log(U) / alpha].  At alpha = 0.03
// U^(1/alpha) is below the smallest float for most U, and a vector whose gammas all underflow has no normalisation; the logarithms
// are ordinary numbers (>= -600), and eta_m = exp(lg_m - max lg) / sum always has a 1.0 in its sum.  The sum is taken in double, so
// the 43 roundings to float leave |sum eta - 1| <= 2^-24.
#pragma once
#include "azr_tree.hpp"

namespace azr {

constexpr float DIR_ALPHA_MAX = 10.0f;   // azr_selfplay_set_dirichlet / azr_debug_root_noise refuse more

// 32-bit integer hash (two multiply-xorshift rounds; full avalanche)
__device__ __forceinline__ uint32_t noise_mix(uint32_t x)
{
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}

// the next uniform of the stream `key`, in (0, 1): (23 random bits + 1/2) * 2^-23, every step exact in fp32
__device__ __forceinline__ float noise_u01(uint32_t key, uint32_t& ctr)
{
    const uint32_t h = noise_mix(key + (ctr++) * 0x9E3779B9u);
    return ((float)(h >> 9) + 0.5f) * (1.0f / 8388608.0f);
}

// log of one Gamma(alpha, 1) variate from the stream `key`
__device__ __forceinline__ float noise_log_gamma(float alpha, uint32_t key)
{
    uint32_t ctr = 0;
    const bool boost = alpha < 1.0f;
    const float a = boost ? alpha + 1.0f : alpha;
    const float d = a - 1.0f / 3.0f;
    const float c = 1.0f / sqrtf(9.0f * d);
    const float logd = logf(d);
    float lg = logd;   // (32 rejections in a row: below 1e-40 at the >= 95 % acceptance of a >= 1; the value d stands in)
    for (int it = 0; it < 32; it++) {
        const float u1 = noise_u01(key, ctr), u2 = noise_u01(key, ctr), u3 = noise_u01(key, ctr);
        const float x = sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
        const float t = 1.0f + c * x;
        if (t <= 0.0f) continue;
        const float v = t * t * t;
        const float logv = logf(v);
        if (logf(u3) < 0.5f * x * x + d - d * v + d * logv) { lg = logd + logv; break; }
    }
    if (boost) lg += logf(noise_u01(key, ctr)) / alpha;
    return lg;
}

// eta[lane] of the root with the legal moves `valid` at decision `decision` of the game with seed `game_seed`; all arguments wave-uniform.
// Not inlined: the tree step and the debug kernel run the same instructions.
__device__ __noinline__ float dirichlet_draw(float alpha, uint32_t noise_seed, uint32_t game_seed, uint32_t decision, uint64_t valid)
{
    const uint32_t l = lane_id();
    valid &= (1ULL << MOVES) - 1ULL;
    if (valid == 0) return 0.0f;
    const bool ok = (valid >> l) & 1ULL;
    uint32_t key = noise_mix(noise_seed + 0x9E3779B9u);
    key = noise_mix(key ^ game_seed);
    key = noise_mix((key ^ decision) + 0x85EBCA6Bu);
    key = noise_mix(key ^ ((l + 1u) * 0x9E3779B9u));
    const float lg = ok ? noise_log_gamma(alpha, key) : -INFINITY;
    const float mx = wave_max(lg);
    const float e = !ok ? 0.0f : lg == mx ? 1.0f : expf(lg - mx);
    double s = (double)e;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    // no gamma left to normalise by (cannot happen in log space unless a logarithm stopped being a number): uniform over the legal moves
    if (!(s >= 1.0) || !(s <= 64.0)) return ok ? 1.0f / (float)popc64(valid) : 0.0f;
    return ok ? (float)((double)e / s) : 0.0f;
}

}  // namespace azr
