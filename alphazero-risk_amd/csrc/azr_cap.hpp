// azr_cap.hpp — playout cap randomisation in device self-play: the coin that makes decision d of a game a FULL decision (the whole
// budget, sampled root noise, one record) or a FAST one (the small budget, the constant noise term, no record).  This engine's own, off
// by default (azr_selfplay_set_playout_cap, include/azr.h); the reference spends MCTS_SIMULATIONS on every decision and records all.
//
// The coin is a function of (cap_seed, game seed, decision, threshold) alone — the counter-based hash of azr_noise.hpp under domain
// constants of its own, so equal seeds do not tie the coin to the Dirichlet draw.  Nothing is taken from the game's minstd_rand0, and
// nothing is stored: whoever needs the kind of the decision in progress recomputes it from the Ctl line's seed and decision count.
// All of it is wave-uniform scalar work.
#pragma once
#include "azr_noise.hpp"

namespace azr {

// full <=> the top 24 bits of the hash fall below `threshold` = (uint32_t)(full_prob * 2^24), computed once on the host in float
__device__ __forceinline__ bool cap_full(uint32_t threshold, uint32_t cap_seed, uint32_t game_seed, uint32_t decision)
{
    uint32_t k = noise_mix(cap_seed + 0xC2B2AE35u);
    k = noise_mix(k ^ game_seed);
    k = noise_mix((k ^ decision) + 0x27D4EB2Fu);
    return (k >> 8) < threshold;
}

}  // namespace azr
