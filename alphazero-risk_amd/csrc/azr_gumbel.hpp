// azr_gumbel.hpp — Gumbel root search with sequential halving (Danihelka, Guez, Schrittwieser, Silver, "Policy improvement by planning
// with Gumbel", ICLR 2022).  This engine's own, off by default (azr_mcts_set_gumbel / azr_selfplay_set_gumbel, include/azr.h states
// every definition); the reference selects by PUCT at every level and records the visit distribution.
//
// At path depth 0 the search visits the root's m best moves by g + logit — g a Gumbel vector drawn per root, so the m moves are a
// sample without replacement from the prior — and halves the set as the budget is spent: the claim with index i goes to a move whose
// search-local visit count equals the considered-visit number cv(i), the best of them by g + logit + sigma(completed Q).  The decision
// plays the most visited of them and records softmax(logit + sigma(completed Q)).  Deeper levels keep tree_select's PUCT, or, in a GTREE step, spend
// their visits in proportion to that softmax of their own rows (gumbel_select_tree, the paper's deterministic non-root selection).
//
// g is a function of (gumbel seed, game seed, decision, move) alone — the counter-based hash of azr_noise.hpp under domain constants of
// its own; nothing is taken from the game's minstd_rand0.  The net's value of a node (vhat) lives in the 44th float of its P row, written
// by the GUMBEL steps where the node is expanded.  Wave-level helpers, lane i <-> move i, fp32 with one rounded operation at a time
// (no contraction), so that tests/gumbel_ref.py restates every number bit for bit.
#pragma once
#include "azr_surprise.hpp"

namespace azr {

constexpr int ND_VHAT = ND_P + MOVES * 4;   // vhat: the padding float behind the node's 43 priors (tree_expand writes 0 there)
constexpr float GUMBEL_FLT_MIN = 1.17549435e-38f;

// e^x for x <= 0: x = k ln 2 + r with k = rint(x / ln 2), |r| <= 0.3466 (ln 2 in two parts, k * the first is exact), e^r as its
// Taylor polynomial to r^7 (Horner), scaled by 2^k in two exact-power steps so that a denormal result is rounded once.  Below -104 the
// result is 0 (e^-104 is less than half the smallest denormal).
__device__ __forceinline__ float exp32(float x)
{
    if (x < -104.0f) return 0.0f;
    const float kf = rintf(__fmul_rn(x, 1.44269502f));
    const int k = (int)kf;
    const float r = __fsub_rn(__fsub_rn(x, __fmul_rn(kf, 0.693145752f)), __fmul_rn(kf, 1.42860682e-06f));
    float p = 1.98412701e-04f;
    p = __fadd_rn(__fmul_rn(p, r), 1.38888892e-03f);
    p = __fadd_rn(__fmul_rn(p, r), 8.33333377e-03f);
    p = __fadd_rn(__fmul_rn(p, r), 4.16666679e-02f);
    p = __fadd_rn(__fmul_rn(p, r), 1.66666672e-01f);
    p = __fadd_rn(__fmul_rn(p, r), 0.5f);
    p = __fadd_rn(__fmul_rn(p, r), 1.0f);
    p = __fadd_rn(__fmul_rn(p, r), 1.0f);
    const int k1 = k >> 1, k2 = k - k1;
    return __fmul_rn(__fmul_rn(p, __uint_as_float((uint32_t)(k1 + 127) << 23)), __uint_as_float((uint32_t)(k2 + 127) << 23));
}

// g[lane] of the root with the legal moves `valid` at decision `decision` of the game with seed `game_seed`; a greedy root (its round
// above temperature_threshold) and the illegal lanes get 0.  All arguments wave-uniform.
__device__ __forceinline__ float gumbel_draw(uint32_t seed, uint32_t game_seed, uint32_t decision, uint64_t valid, bool greedy)
{
    const uint32_t l = lane_id();
    const bool ok = l < (uint32_t)MOVES && ((valid >> l) & 1ULL);
    if (greedy) return 0.0f;
    uint32_t key = noise_mix(seed + 0xB5297A4Du);
    key = noise_mix(key ^ game_seed);
    key = noise_mix((key ^ decision) + 0x1B56C4E9u);
    key = noise_mix(key ^ ((l + 1u) * 0x9E3779B9u));
    uint32_t ctr = 0;
    const float u = noise_u01(key, ctr);
    return ok ? -ln32(-ln32(u)) : 0.0f;
}

// cv(m_eff, n, i): the search-local visit count a move must have to be a candidate of the claim with index i (wave-uniform scalars)
__device__ __forceinline__ uint32_t considered_visit(uint32_t m_eff, uint32_t n, uint32_t i)
{
    if (m_eff <= 1u) return i;
    const uint32_t L = 32u - (uint32_t)__builtin_clz(m_eff - 1u);   // ceil(log2 m_eff)
    uint32_t k = m_eff, base = 0, pos = 0;
    for (;;) {
        const uint32_t q = n / (L * k), e = q > 1u ? q : 1u;
        if (i < pos + e * k) return base + (i - pos) / k;
        pos += e * k;
        base += e;
        k = k / 2u > 2u ? k / 2u : 2u;
    }
}

// qhat[lane]: Q where the move has a completed visit, else v_mix — the net's value vhat of the node mixed with the prior-weighted mean of
// the visited moves' Q.  N: the node's completed visits.  v_mix (wave-uniform) goes out through `v_mix`.
__device__ __forceinline__ float completed_q(uint32_t N, float Q, float P, float vhat, uint64_t valid, float& v_mix)
{
    const uint32_t l = lane_id();
    const bool ok = l < (uint32_t)MOVES && ((valid >> l) & 1ULL);
    const bool seen = ok && N > 0u;
    const float tp = seen ? P : 0.0f;
    const float tq = seen ? __fmul_rn(P, Q) : 0.0f;
    const uint32_t total = wave_sum_u32(ok ? N : 0u);
    float wp = 0.0f, wq = 0.0f;   // a move that does not count adds +0.0f, which leaves a sum that started at +0.0f as it is
#pragma unroll
    for (uint32_t a = 0; a < (uint32_t)MOVES; a++) {
        wp = __fadd_rn(wp, rdlf(tp, a));
        wq = __fadd_rn(wq, rdlf(tq, a));
    }
    v_mix = vhat;
    if (total > 0u && wp > 0.0f) {
        const float fn = (float)total;
        v_mix = __fdiv_rn(__fadd_rn(vhat, __fmul_rn(fn, __fdiv_rn(wq, wp))), __fadd_rn(1.0f, fn));
    }
    return seen ? Q : v_mix;
}

// x[lane] = logit + sigma(qhat) of a root, and qhat through `qhat`; the score of a selection or a decision is (g + logit) + sigma
struct GumbelScore { float logit, sigma, qhat; };
__device__ __forceinline__ GumbelScore gumbel_score(uint32_t N, float Q, float P, float vhat, uint64_t valid, float c_visit, float c_scale)
{
    const uint32_t l = lane_id();
    const bool ok = l < (uint32_t)MOVES && ((valid >> l) & 1ULL);
    GumbelScore s;
    float v_mix;
    s.qhat = completed_q(N, Q, P, vhat, valid, v_mix);
    const uint32_t top = wave_max_u32(ok ? N : 0u);
    s.sigma = __fmul_rn(__fmul_rn(__fadd_rn(c_visit, (float)top), c_scale), s.qhat);
    s.logit = ln32(P < GUMBEL_FLT_MIN ? GUMBEL_FLT_MIN : P);
    return s;
}

// the candidate with the largest score, lowest index on ties; NONE where no candidate's score is a number
__device__ __forceinline__ uint32_t gumbel_best(bool cand, float score)
{
    const float best = wave_max(cand ? score : -INFINITY);
    const uint64_t ties = ballot64(cand && score == best && score > -INFINITY);
    return ties ? (uint32_t)ctz64(ties) : (uint32_t)NONE;
}

// The root-level selection of the claim with index i: W the node's N word (completed visits | in-flight count << 24), N0 the root's
// completed visits when this search began, m the number of moves to consider, n the search's budget.  Returns the move; cv through `cv`.
__device__ __forceinline__ uint32_t gumbel_select(uint32_t W, uint32_t N0, float Q, float P, float g, float vhat, uint64_t valid, uint32_t i,
                                                  uint32_t m, uint32_t n, float c_visit, float c_scale, uint32_t& cv)
{
    const uint32_t l = lane_id();
    const bool ok = l < (uint32_t)MOVES && ((valid >> l) & 1ULL);
    const uint32_t N = W & N_MASK, act = W >> 24;
    const uint32_t legal = (uint32_t)popc64(valid & ((1ULL << MOVES) - 1ULL));
    cv = considered_visit(m < legal ? m : legal, n, i);
    const uint32_t cnt = (N > N0 ? N - N0 : 0u) + act;
    bool cand = ok && cnt == cv;
    if (ballot64(cand) == 0) {   // nobody stands at cv: the moves closest below it ...
        const bool below = ok && cnt < cv;
        const uint32_t top = wave_max_u32(below ? cnt + 1u : 0u);
        cand = below && cnt + 1u == top;
        if (ballot64(cand) == 0) cand = ok;   // ... and, at a root a transposition visited from below, every legal move
    }
    const GumbelScore s = gumbel_score(N, Q, P, vhat, valid, c_visit, c_scale);
    return gumbel_best(cand, __fadd_rn(__fadd_rn(g, s.logit), s.sigma));
}

// the record's pi[lane] from the root's score s: softmax(logit + sigma) over the legal moves, the sum taken one after the other in
// index order
__device__ __forceinline__ float gumbel_policy(const GumbelScore& s, uint64_t valid, float* qhat = nullptr)
{
    const uint32_t l = lane_id();
    const bool ok = l < (uint32_t)MOVES && ((valid >> l) & 1ULL);
    if (qhat) *qhat = ok ? s.qhat : 0.0f;
    const float x = __fadd_rn(s.logit, s.sigma);
    const float mx = wave_max(ok ? x : -INFINITY);
    const float e = ok ? exp32(__fsub_rn(x, mx)) : 0.0f;
    float sum = 0.0f;
#pragma unroll
    for (uint32_t a = 0; a < (uint32_t)MOVES; a++) sum = __fadd_rn(sum, rdlf(e, a));
    return ok ? __fdiv_rn(e, sum) : 0.0f;
}

// the decision's move from the root's score s: the legal move with the most search-local visits, the best of them by g + logit + sigma
__device__ __forceinline__ uint32_t gumbel_move(const GumbelScore& s, uint32_t N, uint32_t N0, float g, uint64_t valid)
{
    const uint32_t l = lane_id();
    const bool ok = l < (uint32_t)MOVES && ((valid >> l) & 1ULL);
    if ((valid & ((1ULL << MOVES) - 1ULL)) == 0) return NONE;
    const uint32_t ns = N > N0 ? N - N0 : 0u;
    const uint32_t top = wave_max_u32(ok ? ns + 1u : 0u);
    return gumbel_best(ok && ns + 1u == top, __fadd_rn(__fadd_rn(g, s.logit), s.sigma));
}

// vhat of node idx (wave-uniform), and its store where consume_pending has expanded the node
__device__ __forceinline__ float node_vhat(const Tree& t, uint32_t idx) { return rdlf(*reinterpret_cast<const float*>(node_ptr(t, idx) + ND_VHAT), 0); }
__device__ __forceinline__ void node_set_vhat(const Tree& t, uint32_t idx, float v)
{
    if (lane_id() == 0) *reinterpret_cast<float*>(node_ptr(t, idx) + ND_VHAT) = v;
    wave_mem_sync();
}

// tree_select's place at path depth 0 of a GUMBEL step: the selection above on node idx, with tree_select's bookkeeping (touch stamp,
// active_N++ on the chosen move).  n0: the game's N0 row; the claim with index 0 — the search's first root-level selection — takes
// the snapshot.
__device__ __forceinline__ uint32_t gumbel_select_root(const Tree& t, uint32_t idx, const NodeRegs& nr, uint32_t stamp, uint32_t* n0, uint32_t i,
                                                       uint32_t m, uint32_t n, float c_visit, float c_scale, float g)
{
    const uint8_t* nd = node_ptr(t, idx);
    const uint32_t l = lane_id(), ll = l < (uint32_t)MOVES ? l : 0u;
    const uint64_t valid = (uint64_t)rfl(nr.valid_lo) | ((uint64_t)rfl(nr.valid_hi) << 32);
    const uint32_t W = nr.W;
    if (l == 0) t.touch[idx] = stamp;
    uint32_t N0 = W & N_MASK;
    if (i == 0) { if (l < (uint32_t)MOVES) n0[l] = N0; }
    else N0 = n0[ll];
    uint32_t cv;
    const uint32_t mv = gumbel_select(W, N0, nr.Q, nr.P, g, node_vhat(t, idx), valid, i, m, n, c_visit, c_scale, cv);
    if (mv != NONE && l == mv) reinterpret_cast<uint32_t*>(const_cast<uint8_t*>(nd) + ND_N)[l] = W + ACT_ONE;
    wave_mem_sync();
    return mv;
}

// tree_select's place at path depth >= 1 of a GTREE step: the node's visits follow pi' = gumbel_policy of its own rows (W its N word),
// the move = the legal one with the largest pi' - cnt / (1 + sum cnt), cnt the completed visits and those in flight.  Nothing is drawn.
// nrow, touch: the node's N row and touch stamp for tree_select's bookkeeping (stamp, active_N++ on the chosen move); both null on
// synthetic rows.  score[lane] goes out through `score_out` where somebody asks, 0 on an illegal move.
__device__ __forceinline__ uint32_t gumbel_select_tree(uint32_t W, float Q, float P, float vhat, uint64_t valid, float c_visit, float c_scale,
                                                       uint32_t* nrow, uint32_t* touch, uint32_t stamp, float* score_out = nullptr)
{
    const uint32_t l = lane_id();
    const bool ok = l < (uint32_t)MOVES && ((valid >> l) & 1ULL);
    if (touch && l == 0) *touch = stamp;
    const float pi = gumbel_policy(gumbel_score(W & N_MASK, Q, P, vhat, valid, c_visit, c_scale), valid);
    const uint32_t cnt = (W & N_MASK) + (W >> 24);
    const float den = __fadd_rn(1.0f, (float)wave_sum_u32(ok ? cnt : 0u));
    const float score = __fsub_rn(pi, __fdiv_rn((float)cnt, den));
    if (score_out) *score_out = ok ? score : 0.0f;
    const uint32_t mv = gumbel_best(ok, score);
    if (nrow) {
        if (mv != NONE && l == mv) nrow[l] = W + ACT_ONE;
        wave_mem_sync();
    }
    return mv;
}

}  // namespace azr
