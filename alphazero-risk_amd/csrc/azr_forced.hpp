// azr_forced.hpp — forced playouts and policy target pruning at the root of a self-play search (Wu, "Accelerating Self-Play Learning in
// Go", 2019, section 3.2).  This engine's own, off by default (azr_mcts_set_forced_playouts / azr_selfplay_set_forced_playouts,
// include/azr.h states both definitions); the reference has neither.
//
// Forced playouts: at path depth 0 a root child that has been tried (N > 0) is selected until N reaches nf = sqrt(k * noiseP * sumN),
// whatever PUCT thinks of it.  Policy target pruning: where a record's pi is computed, the forced visits PUCT would not have spent on
// its own are subtracted again — each child other than the most visited one gives back visits, at most trunc(nf) of them, while its
// PUCT score at the reduced count stays below the most visited child's; a child reduced to one visit goes to zero.
//
// Both are wave-level helpers, lane i <-> move i, fp32 with the intrinsics and the operation order of tree_select (no contraction).
#pragma once
#include "azr_wave.hpp"

namespace azr {

constexpr float FORCED_K_MAX = 8.0f;   // azr_*_set_forced_playouts reject a larger factor (KataGo runs k = 2)

__device__ __forceinline__ float forced_nf(float k, float noiseP, uint32_t sumN)
{
    return sqrtf(__fmul_rn(__fmul_rn(k, noiseP), (float)sumN));
}

// a legal move that has been tried and is still short of its forced count (a NaN nf — negative noiseP — forces nothing)
__device__ __forceinline__ bool forced_move(bool legal, uint32_t N, float nf) { return legal && N > 0 && (float)N < nf; }

// trunc(nf) as the pruning's cap on what a child may give back: 0 for a NaN or non-positive nf, saturated at 2^24 - 1 (no count is larger)
__device__ __forceinline__ uint32_t forced_cap(float nf) { return !(nf > 0.0f) ? 0u : (nf >= 16777215.0f ? 16777215u : (uint32_t)nf); }

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, m); v = o > v ? o : v; }
    return v;
}

// N' of the root's children (lane = move): N, Q and noiseP of this lane's move, `valid` and `sumN` of the node, k > 0 the forcing
// factor, hp the PUCT constant.  The loop is the definition (include/azr.h); it runs in lock-step over the lanes and ends after at most
// max trunc(nf) rounds.  Lanes of illegal moves and lanes >= 43 return their N unchanged.
__device__ __forceinline__ uint32_t prune_counts(uint32_t N, float Q, float noiseP, uint64_t valid, uint32_t sumN, float k, float hp)
{
    const uint32_t l = lane_id();
    const bool ok = l < (uint32_t)MOVES && ((valid >> l) & 1ULL);
    if (valid == 0) return N;
    const float v = __fmul_rn(__fmul_rn(noiseP, hp), sqrtf(__fadd_rn(1.0f, (float)sumN)));
    const uint32_t top = wave_max_u32(ok ? N : 0u);
    const uint32_t cstar = (uint32_t)ctz64(ballot64(ok && N == top));   // the most visited legal move, lowest index on ties
    const float ustar = rdlf(__fadd_rn(Q, __fdiv_rn(v, __fadd_rn(1.0f, (float)N))), cstar);
    const uint32_t f = forced_cap(forced_nf(k, noiseP, sumN));
    const uint32_t lower = N > f ? N - f : 0u;
    const bool mine = ok && l != cstar && N > 0;
    uint32_t Np = N;
    for (;;) {
        const bool more = mine && Np > lower && __fadd_rn(Q, __fdiv_rn(v, __fadd_rn(1.0f, (float)(Np - 1u)))) < ustar;
        if (ballot64(more) == 0) break;
        if (more) Np--;
    }
    if (mine && Np == 1u && Np < N) Np = 0u;   // reduced to a single playout: pruned outright
    return Np;
}

}  // namespace azr
