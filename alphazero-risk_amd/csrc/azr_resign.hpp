// azr_resign.hpp — resignation in device self-play with a no-resign holdout (AlphaGo Zero, KataGo).  This engine's own, off by default
// (azr_selfplay_set_resign, include/azr.h states the rule); the reference plays every game to its last dice roll.
//
// A player whose root value q stays below q_resign for `streak` of its own recorded decisions in a row gives the game up: the game ends
// there as a win for the opponent and its staged records are flushed as after any end.  A share of the games, chosen by a coin of
// (seed, game seed), is held out: such a game never resigns, plays on, and reports at its natural end whether the player who would
// have resigned first went on not to lose — the rule's false positives.
//
// The state of a running game is one uint32 beside the staging buffer (Dev::resign_state): run[0] in bits 0..7, run[1] in bits 8..15,
// `first` in bits 16..17 (0 = none, 1 + p otherwise); zero when a game starts.  The coin is recomputed from the Ctl line's seed and
// never stored.  All of it is wave-uniform scalar work; the state update and the coin are stated here once, for the self-play step and
// for k_debug_resign.
#pragma once
#include "azr_internal.hpp"
#include "azr_noise.hpp"

namespace azr {

constexpr uint32_t RESIGN_FIRST_SHIFT = 16, RESIGN_FIRST_MASK = 3u << RESIGN_FIRST_SHIFT;

// held out <=> the top 24 bits of the hash fall below `threshold` = (uint32_t)(holdout_share * 2^24), computed once on the host in
// float.  The two constants are none of the Dirichlet sampler's, the playout cap's or the copy coin's.
__device__ __forceinline__ bool resign_holdout(uint32_t threshold, uint32_t seed, uint32_t game_seed)
{
    uint32_t k = noise_mix(seed + 0x2545F491u);
    k = noise_mix(k ^ game_seed);
    k = noise_mix(k + 0x68E31DA4u);
    return (k >> 8) < threshold;
}

// One decision of player p (0 / 1) with the root value q: run[p] grows by one below the bound (saturating at 255) and falls to zero
// otherwise; the other player's run is untouched.  True: p gives up (run[p] >= streak).
__device__ __forceinline__ bool resign_update(uint32_t& state, uint32_t p, float q, bool has_q, float q_resign, uint32_t streak)
{
    const uint32_t sh = p * 8u;
    uint32_t run = (state >> sh) & 255u;
    const bool below = has_q && q < q_resign;
    run = below ? (run < 255u ? run + 1u : 255u) : 0u;
    state = (state & ~(255u << sh)) | (run << sh);
    return run >= streak;
}

// `first` of a state: 255 = none, else the player who would have resigned first
__device__ __forceinline__ uint32_t resign_first(uint32_t state)
{
    const uint32_t f = (state & RESIGN_FIRST_MASK) >> RESIGN_FIRST_SHIFT;
    return f ? f - 1u : 255u;
}
// a held-out game's player p gives up: remembered if nobody has before
__device__ __forceinline__ void resign_note_first(uint32_t& state, uint32_t p)
{
    if (!(state & RESIGN_FIRST_MASK)) state |= (p + 1u) << RESIGN_FIRST_SHIFT;
}

// The statistics row of slot g ({resigned, holdout_games, holdout_would_resign, holdout_not_lost}) after a game that did not end on a
// rules error: a resignation, or the natural end with `status` of a game that is held out or not.  Lane i < 4 owns word i: the slot's
// own wave, no atomics; the host sums the rows.
__device__ __forceinline__ void resign_count_game(const Dev& E, int g, uint32_t state, bool resigned, bool holdout, int status)
{
    const uint32_t first = resign_first(state);
    const bool would = first != 255u;
    const uint32_t l = lane_id();
    bool bump = false;
    bump = l == 0 ? resigned : bump;
    bump = l == 1 ? (!resigned && holdout) : bump;
    bump = l == 2 ? (!resigned && holdout && would) : bump;
    bump = l == 3 ? (!resigned && holdout && would && status != 1 - (int)first) : bump;
    if (l < 4 && bump) E.resign_stats[(size_t)g * 4 + l] += 1ull;
}

}  // namespace azr
