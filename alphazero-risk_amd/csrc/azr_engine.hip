// azr_engine.hip — kernels and C-ABI (include/azr.h) of the batched Risk state-step + flattened MCTS.
// One wavefront per game; grid = G workgroups of 64 threads.  gfx950 only.
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <new>

#include "azr_arena.hpp"

using namespace azr;

// ================================================================================================
// rules kernels (UtilityNN / State seams)
// ================================================================================================
__global__ __launch_bounds__(64) void k_new_games(Dev E, const uint32_t* seeds)
{
    const int g = blockIdx.x;
    WS s;
    ws_blank(s);
    s.rng = rng_seed(rfl(seeds[g]));
    new_game(s);
    ws_store(s, E.state + (size_t)g * GREC);
    if (lane_id() == 0) E.ctl[g].rng = s.rng;
}

__global__ __launch_bounds__(64) void k_valid_moves(Dev E, uint64_t* out)
{
    const int g = blockIdx.x;
    WS s;
    ws_load(s, E.state + (size_t)g * GREC);
    uint64_t vm = valid_moves(s, E.rules);
    if (lane_id() == 0) out[g] = vm;
}

__global__ __launch_bounds__(64) void k_make_moves(Dev E, const uint8_t* moves, uint8_t* rc)
{
    const int g = blockIdx.x;
    const uint32_t mv = rfl(moves[g]);
    if (mv == 255u) {
        if (lane_id() == 0) rc[g] = 0;
        return;
    }
    WS s;
    ws_load(s, E.state + (size_t)g * GREC);
    s.rng = rfl(E.ctl[g].rng);
    make_move(s, mv, E.rules);
    if (s.err == 0) {  // a throwing move leaves the stored game untouched
        ws_store(s, E.state + (size_t)g * GREC);
        if (lane_id() == 0) E.ctl[g].rng = s.rng;
    }
    if (lane_id() == 0) rc[g] = (uint8_t)s.err;
}

__global__ __launch_bounds__(64) void k_status(Dev E, int8_t* out)
{
    const int g = blockIdx.x;
    WS s;
    ws_load(s, E.state + (size_t)g * GREC);
    int st = game_status(s, E.rules);
    if (lane_id() == 0) out[g] = (int8_t)st;
}

__global__ __launch_bounds__(64) void k_encode(Dev E, uint8_t* out /*[G][88]*/)
{
    const int g = blockIdx.x;
    WS s;
    ws_load(s, E.state + (size_t)g * GREC);
    encode88(s, out + (size_t)g * 88);
}

// reference `Data` image (160 B) -> 64-B record.  The five masks / totalArmy of the image are derived data and
// are ignored on import (recomputed on export).
// the byte of the 64-B record this lane holds, from the image `d`
__device__ __forceinline__ uint32_t import160_byte(const uint8_t* d)
{
    const uint32_t l = lane_id();
    uint32_t b = 0;
    if (l < LANDS) b = d[l];
    b = l == GR_CUR ? d[146] : b;
    b = l == GR_CARD_SETS ? d[147] : b;
    b = l == GR_REINF ? d[148] : b;
    b = l == GR_PHASE ? d[149] : b;
    b = l == GR_MOB_FROM ? d[150] : b;
    b = l == GR_MOB_TO ? d[151] : b;
    b = l == GR_ALLOW_DRAW ? d[152] : b;
    b = l == GR_ATTACKS ? d[153] : b;
    b = l == GR_ROUND_LO ? d[144] : b;
    b = l == GR_ROUND_HI ? d[145] : b;
    b = l == GR_CARDS0 ? d[48 + 40] : b;
    b = l == GR_CARDS1 ? d[96 + 40] : b;
    return b;
}
__global__ __launch_bounds__(64) void k_import160(Dev E, const uint8_t* data160)
{
    const int g = blockIdx.x;
    E.state[(size_t)g * GREC + lane_id()] = (uint8_t)import160_byte(data160 + (size_t)g * 160);
}

__global__ __launch_bounds__(64) void k_export160(Dev E, const uint8_t* records, uint8_t* data160)
{
    const int g = blockIdx.x;
    uint8_t* d = data160 + (size_t)g * 160;
    const uint32_t l = lane_id();
    WS s;
    ws_load(s, records + (size_t)g * GREC);
    for (uint32_t i = l; i < 160; i += 64) d[i] = 0;
    wave_mem_sync();
    if (l < LANDS) d[l] = (uint8_t)s.la;
    for (uint32_t p = 0; p < 2; p++) {
        uint64_t m[5] = {m_owned(s, p), m_owned_army(s, p), m_owned_full(s, p), m_attack(s, p), m_attack_army(s, p)};
        int ta = total_army(s, p);
        uint8_t* q = d + 48 + 48 * p;
        if (l < 30) {  // 5 masks x 6 bytes
            uint32_t k = l / 6, by = l % 6;
            q[8 * k + by] = (uint8_t)(m[k] >> (8 * by));
        }
        if (l == 30) q[38] = (uint8_t)(ta & 0xff);
        if (l == 31) q[39] = (uint8_t)((ta >> 8) & 0xff);
        if (l == 32) q[40] = (uint8_t)cards_of(s, p);
    }
    if (l == 0) {
        d[144] = (uint8_t)(s.round & 0xff); d[145] = (uint8_t)(s.round >> 8); d[146] = (uint8_t)s.cur;
        d[147] = (uint8_t)s.card_sets; d[148] = (uint8_t)s.reinf; d[149] = (uint8_t)s.phase;
        d[150] = (uint8_t)s.mob_from; d[151] = (uint8_t)s.mob_to; d[152] = (uint8_t)s.allow_draw;
        d[153] = (uint8_t)s.attacks;
    }
}

// ================================================================================================
// search kernels
// ================================================================================================
__global__ __launch_bounds__(64) void k_tree_clear(Dev E)
{
    const int g = blockIdx.x;
    Ctl c;
    ctl_load(c, &E.ctl[g]);
    Tree t = tree_of(E, g);
    // hiwater may be stale at creation: clear everything the pool can hold
    c.hiwater = (uint32_t)E.C;
    tree_clear(t, c);
    c.pending = 0; c.sims_started = 0; c.sims_done = 0; c.search_done = 1;
    ctl_store(c, &E.ctl[g]);
}

__global__ __launch_bounds__(64) void k_tree_trim(Dev E)
{
    const int g = blockIdx.x;
    Ctl c;
    ctl_load(c, &E.ctl[g]);
    Tree t = tree_of(E, g);
    tree_trim(t, c);
    ctl_store(c, &E.ctl[g]);
}

// AlphaZeroMCTS::simulate prologue (setRootState's trimNodes) for host-stepped searches
__global__ __launch_bounds__(64) void k_search_begin(Dev E)
{
    const int g = blockIdx.x;
    Ctl c;
    ctl_load(c, &E.ctl[g]);
    Tree t = tree_of(E, g);
    WS s;
    ws_load(s, E.state + (size_t)g * GREC);
    tree_trim(t, c);
    c.mode = 1;
    c.sims_done = 0; c.sims_started = 0; c.pending = 0; c.error = 0;
    c.search_done = game_status(s, E.rules) != ST_NOT_ENDED ? 1u : 0u;
    ctl_store(c, &E.ctl[g]);
}

// One tree step for game g: consume the pending leaf's (pi, v) [expand + backup], then run searches — and in
// self-play mode decisions, moves and game restarts — until the next leaf that needs the net.
// NOISE: root noise is in force (host-stepped: azr_mcts_set_root_noise's vector; self-play: a Dirichlet draw per new root).  The
// default instantiations carry none of it.
// CAP (self-play only): a playout cap is in force (azr_selfplay_set_playout_cap).  The decision in progress is full or fast by the coin
// of (cap seed, game seed, decision) — recomputed here from the Ctl line, never stored; a fast decision searches E.cap_fast descents
// with the constant root vector and stages no record.  Everything else — trim, pick, move, turnover, z back-fill — is the same code.
// FORCED (with NOISE only; a search without a sampled vector runs on the constant one, which is the constant form bit for bit): forced
// playouts at path depth 0 with the factor E.forced_k (azr_forced.hpp) — not in a fast decision; with E.prune the staged record's pi
// comes from the pruned counts N', the move still from N.
// SURPRISE (self-play only): policy surprise weighting of the records (azr_surprise.hpp) — KL(pi || P) of every staged record is kept
// beside it, and a finished game's records are written floor(w) or ceil(w) times each by flush_samples_weighted.  The search, the moves
// and the staged records are the ones without it.
// QMIX (self-play only): the value mix of the records (azr_valuemix.hpp) — the root value q of every staged record, from the root's
// unpruned N and its Q, is kept beside it, and both flush paths write z' = (1 - q_share) z + q_share q in place of z.  The search, the
// moves, pi, the copies and every counter are the ones without it.
// Resignation (self-play only; azr_resign.hpp) is no template argument: E.resign_streak is wave-uniform and read once per decision.  On,
// a recorded decision updates the mover's run from the root value after its record is staged; a run that reaches the streak ends the
// game there for the opponent, or, in a held-out game, is only remembered.  Off, the decision is the one without it.
// GUMBEL (without NOISE, CAP and FORCED): the Gumbel root search (azr_gumbel.hpp) — at path depth 0 the descents select by
// gumbel_select_root under the root's vector g (E.root_g; self-play: a draw per new root), an expanded node keeps the net's value, and
// a self-play decision takes gumbel_move and stages gumbel_policy, without an rFloat.  Staging, z back-fill, turnover, quota, surprise
// weighting, value mix and resignation work on what they are handed.
// GTREE (with GUMBEL only): below the root the descents select by gumbel_select_tree, the improved policy of each node's own rows, in
// place of tree_select's PUCT; the root-level selection, the decision and the record are GUMBEL's.
template <bool SELFPLAY, bool NOISE, bool CAP, bool FORCED, bool SURPRISE = false, bool QMIX = false, bool GUMBEL = false, bool GTREE = false>
__global__ __launch_bounds__(64) void k_tree_step(Dev E)
{
    static_assert((SELFPLAY || !CAP) && (NOISE || !FORCED) && (SELFPLAY || !SURPRISE) && (SELFPLAY || !QMIX) && (!GUMBEL || (!NOISE && !CAP && !FORCED)) &&
                      (GUMBEL || !GTREE),
                  "CAP, SURPRISE and QMIX need SELFPLAY, FORCED implies NOISE, GUMBEL excludes NOISE, CAP and FORCED, GTREE needs GUMBEL: launch_tree_step lists the thirty-seven");
    __shared__ int8_t scratch[128];
    const int g = blockIdx.x;
    TP_BEGIN();
    Ctl c;
    ctl_load(c, &E.ctl[g]);
    if (c.mode == 0 || (!SELFPLAY && c.search_done)) return;
    const unsigned long long cnt0 = counters_begin(E, g);
    Tree t = tree_of(E, g);
    const Rules R = E.rules;
    const Search S = E.search;
    // the budget of the decision in progress: S's own without a cap, else by the decision's kind (re-derived after every decision and
    // every new game, below)
    Search Sd = S;
    bool full = true;
    if (CAP) { full = cap_full(E.cap_threshold, E.cap_seed, c.seed, c.decisions); Sd.simulations = full ? S.simulations : E.cap_fast; }
    WS root;
    ws_load(root, E.state + (size_t)g * GREC);
    StepCount k;
    bool root_dirty = false;
    float eta = 0.0f;
    if (NOISE) eta = E.root_eta[(size_t)g * MOVES + (lane_id() < MOVES ? lane_id() : 0)];
    if (FORCED && !SELFPLAY && E.eta_const) eta = E.noise_value;   // host-stepped, no vector set: the constant form
    if (GUMBEL) eta = E.root_g[(size_t)g * MOVES + (lane_id() < MOVES ? lane_id() : 0)];   // the root's g travels where eta would
    TP(0);
    consume_pending<GUMBEL>(E, g, t, c, k);
    for (;;) {
        TP(6);
        if ((int)c.sims_done >= (CAP ? Sd.simulations : S.simulations)) {
            if (!SELFPLAY) { c.search_done = 1; break; }
            // ---- one decision of the trainer's move loop (alphazero_trainer.cpp:91-112) ----
            root.rng = c.rng;
            uint32_t N; uint64_t valid;
            uint32_t mv = NONE;
            float P = 0.0f;   // SURPRISE: the root's stored prior row
            float Q = 0.0f;   // QMIX, resignation: the root's mean values
            // resignation (azr_resign.hpp): a runtime setting, wave-uniform, looked at here once per decision; off, nothing below runs
            const bool resign = E.resign_streak > 0;
            const uint32_t mover = root.cur;
            uint32_t rs = 0;          // the running game's runs and `first`
            bool resigned = false;    // the mover gives the game up at this decision
            if (resign) rs = rfl(E.resign_state[g]);
            if (root_node(t, root, N, valid, (GUMBEL || QMIX || resign) ? &Q : nullptr, (GUMBEL || SURPRISE) ? &P : nullptr) != NO_NODE) {
                float pi;
                if (GUMBEL) {   // no rFloat: the move is a function of the search and g; one score serves the move and the record
                    // (the node is looked up again, as for the pruned counts below: keeping root_node's index in a variable, in any form,
                    //  moves one s_mov in three of the existing SURPRISE steps, and those stay the parent's instruction for instruction)
                    const uint32_t rkd = ws_record_dword(root);
                    const uint32_t ridx = tree_lookup(t, rkd, key_hash(t, rkd));
                    const GumbelScore sc = gumbel_score(N, Q, P, node_vhat(t, ridx), valid, E.gumbel_cvisit, E.gumbel_cscale);
                    mv = gumbel_move(sc, N, E.root_n0[(size_t)g * MOVES + (lane_id() < MOVES ? lane_id() : 0)], eta, valid);
                    pi = gumbel_policy(sc, valid);
                } else {
                    pi = root_policy(N, valid);
                    mv = (int)root.round > S.temperature_threshold ? pick_highest(pi) : pick_random(root, pi);
                }
                if (FORCED && E.prune && (!CAP || full)) {   // the record's pi from N'; the move above is N's
                    const uint32_t rkd = ws_record_dword(root);
                    pi = root_policy(root_pruned_counts(E, S, t, tree_lookup(t, rkd, key_hash(t, rkd)), N, valid, eta, E.forced_k), valid);
                }
                if (SURPRISE && (!CAP || full)) stage_surprise(E, g, c, pi, P, valid);
                if (QMIX && (!CAP || full)) stage_root_value(E, g, c, N, Q, valid);   // N is the unpruned count
                if (!CAP || full) stage_sample(E, g, c, root, pi, k);
                if (resign && (!CAP || full)) resigned = resign_decision(E, g, c, rs, mover, N, Q, valid);
            }
            TP(16);
            if (resigned) { mv = NONE; root.rng = c.rng; }   // no pick, no rFloat (the pick's above is taken back), no move: the game ends at this root
            else if (mv != NONE) make_move(root, mv, R); else root.err = E_LOGIC;
            c.last_move = mv;
            c.decisions++;
            k.dec++;
            c.rng = root.rng;
            int st = resigned ? 1 - (int)mover /* a win for the opponent */ : root.err ? ST_NOT_ENDED : game_status(root, R);
            TP(17);
            if (root.err || st != ST_NOT_ENDED) {
                if (root.err) { k.err++; c.error = root.err; }
                else {
                    wave_mem_sync();
                    if (SURPRISE) k.samples += flush_samples_weighted<QMIX>(E, g, c.nsamples, st, c.seed, k.ringdrop);
                    else {
                        flush_samples<QMIX>(E, g, c.nsamples, st, k.ringdrop);
                        k.samples += c.nsamples;
                    }
                    k.games++;
                    if (resign) resign_count_game(E, g, rs, resigned, !resigned && resign_holdout(E.resign_threshold, E.resign_seed, c.seed), st);
                }
                c.status = st;
                selfplay_next_game(E, g, t, c, root);
            }
            root_dirty = true;
            TP(18);
            if (CAP) { full = cap_full(E.cap_threshold, E.cap_seed, c.seed, c.decisions); Sd.simulations = full ? S.simulations : E.cap_fast; }
            if (NOISE) eta = new_root_noise<CAP, FORCED>(E, g, c, root, full);   // the next decision's root, or the next game's first
            if (GUMBEL) eta = new_root_gumbel(E, g, c, root);
            if (c.mode == 0) break;  // quota exhausted: the slot idles
            tree_trim(t, c);
            c.sims_done = 0; c.sims_started = 0;
            TP(14);
        }
        uint32_t err = 0;
        int r = search_round<NOISE, FORCED, GUMBEL, GTREE>(E, CAP ? Sd : S, g, t, c, root, scratch, k, err, eta, (FORCED && (!CAP || full)) ? E.forced_k : 0.0f);
        if (r == RD_LEAF) break;
        if (r == RD_FAIL) {
            k.err++;
            c.error = err;
            if (SELFPLAY) {  // abandon the game (the reference would have thrown): restart the slot
                selfplay_next_game(E, g, t, c, root);
                root_dirty = true;
                if (CAP) { full = cap_full(E.cap_threshold, E.cap_seed, c.seed, c.decisions); Sd.simulations = full ? S.simulations : E.cap_fast; }
                if (NOISE) eta = new_root_noise<CAP, FORCED>(E, g, c, root, full);
                if (GUMBEL) eta = new_root_gumbel(E, g, c, root);
                if (c.mode == 0) break;
                tree_trim(t, c);
                continue;
            }
            c.search_done = 1;
            break;
        }
    }
    TP(6);
    if (root_dirty) ws_store(root, E.state + (size_t)g * GREC);
    TP(19);
    ctl_store(c, &E.ctl[g]);
    TP(20);
    flush_counters(E, g, c, k, !SELFPLAY, cnt0);
    TP(21);
    // self-play tail (quota mode, slots going idle): the net of this pass runs on the waiting leaf slots only
    if (SELFPLAY && E.sp_compact) list_pending(E, g, c, &E.leaf_count[0], E.leaf_list);
    TP(15);
    TP_END();
}

__global__ __launch_bounds__(64) void k_arena_step(Dev E)
{
    __shared__ int8_t scratch[128];
    arena_step<false>(E, scratch);
}
__global__ __launch_bounds__(64) void k_arena_step_rec(Dev E)
{
    __shared__ int8_t scratch[128];
    arena_step<true>(E, scratch);
}
// an AlphaZero side of the arena searches by the Gumbel root search (azr_arena_set_gumbel)
__global__ __launch_bounds__(64) void k_arena_step_gumbel(Dev E, ArenaGumbel A)
{
    __shared__ int8_t scratch[128];
    arena_step<false, true>(E, scratch, &A);
}

__global__ __launch_bounds__(64) void k_arena_start(Dev E)
{
    const int g = blockIdx.x;
    Ctl c;
    ctl_load(c, &E.ctl[g]);
    Tree t = tree_of(E, g);
    c.hiwater = (uint32_t)E.C;
    tree_clear(t, c);
    if (E.nodes2) {  // the opponent player's tree starts empty with its own stamp counter
        Ctl c2 = c;
        c2.hiwater = (uint32_t)E.C;
        tree_clear(tree2_of(E, g), c2);
        if (lane_id() == 0) { uint32_t* d2 = E.tctl2 + (size_t)g * 4; d2[0] = c2.search_id; d2[1] = c2.nfree; d2[2] = c2.hiwater; d2[3] = 0; }
    }
    c.search_tree = 0; c.nsamples = 0;
    c.mode = 3; c.sims_done = 0; c.sims_started = 0; c.pending = 0; c.search_done = 0; c.error = 0;
    c.arena_state = 0; c.player_start = 0; c.pair_phase = 0; c.turn_started = 0; c.search_active = 0; c.slot_games = 0;
    c.seed = E.base_seed + (uint32_t)g;
    c.rng = rng_seed(c.seed);
    ScriptW* dst = reinterpret_cast<ScriptW*>(E.script) + (size_t)g * 2;
    if (lane_id() == 0) { ScriptW w; script_init(w); dst[0] = w; dst[1] = w; }
    ctl_store(c, &E.ctl[g]);
}

// root statistics / policy / pick for host-stepped use
__global__ __launch_bounds__(64) void k_root_stats(Dev E, uint32_t* n_out, float* q_out, float* p_out, float* pi_out)
{
    const int g = blockIdx.x;
    Ctl c;
    ctl_load(c, &E.ctl[g]);
    Tree t = tree_of(E, g);
    WS root;
    ws_load(root, E.state + (size_t)g * GREC);
    uint32_t N; uint64_t valid; float Q = 0, P = 0, pi = 0;
    if (root_node(t, root, N, valid, &Q, &P) != NO_NODE) pi = root_policy(N, valid);
    const uint32_t l = lane_id();
    if (l < MOVES) {
        if (n_out) n_out[(size_t)g * MOVES + l] = N;
        if (q_out) q_out[(size_t)g * MOVES + l] = Q;
        if (p_out) p_out[(size_t)g * MOVES + l] = P;
        if (pi_out) pi_out[(size_t)g * MOVES + l] = pi;
    }
}

// azr_mcts_node_stats: the rows of the node of state g of `data160` in game g's tree; the state lives in registers only, nothing is written
// but the outputs
__global__ __launch_bounds__(64) void k_node_stats(Dev E, const uint8_t* data160, uint32_t* n_out, uint32_t* act_out, float* q_out, float* p_out,
                                                   float* vhat_out, uint8_t* found_out)
{
    const int g = blockIdx.x;
    const Tree t = tree_of(E, g);
    WS s;
    ws_from_byte(s, import160_byte(data160 + (size_t)g * 160));
    const uint32_t kd = ws_record_dword(s);
    const uint32_t idx = tree_lookup(t, kd, key_hash(t, kd));
    const uint32_t l = lane_id(), ll = l < MOVES ? l : 0;
    uint32_t W = 0;
    float Q = 0.0f, P = 0.0f, vhat = 0.0f;
    if (idx != NO_NODE) {
        const uint8_t* n = node_ptr(t, idx);
        W = reinterpret_cast<const uint32_t*>(n + ND_N)[ll];
        Q = reinterpret_cast<const float*>(n + ND_Q)[ll];
        P = reinterpret_cast<const float*>(n + ND_P)[ll];
        vhat = node_vhat(t, idx);
    }
    if (l < MOVES) {
        n_out[(size_t)g * MOVES + l] = W & N_MASK;
        if (act_out) act_out[(size_t)g * MOVES + l] = W >> 24;
        q_out[(size_t)g * MOVES + l] = Q;
        p_out[(size_t)g * MOVES + l] = P;
    }
    if (l == 0) {
        if (vhat_out) vhat_out[g] = vhat;
        found_out[g] = idx != NO_NODE ? 1 : 0;
    }
}

// azr_mcts_root_value: q of the last search's roots by the self-play step's root_value (0 and has_q 0 for a root that is not in the tree)
__global__ __launch_bounds__(64) void k_root_value(Dev E, float* q_out, uint8_t* has_q_out)
{
    const int g = blockIdx.x;
    Ctl c;
    ctl_load(c, &E.ctl[g]);
    Tree t = tree_of(E, g);
    WS root;
    ws_load(root, E.state + (size_t)g * GREC);
    uint32_t N; uint64_t valid; float Q = 0.0f, q = 0.0f;
    bool has_q = false;
    if (root_node(t, root, N, valid, &Q) != NO_NODE) q = root_value(N, Q, valid, has_q);
    if (lane_id() == 0) {
        q_out[g] = q;
        if (has_q_out) has_q_out[g] = has_q ? 1 : 0;
    }
}

// azr_debug_value_mix: the rule alone, one wave per row, through the device functions of the step and its flushes
__global__ __launch_bounds__(64) void k_debug_value_mix(float q_share, const uint32_t* N, const float* Q, const uint64_t* valid, const float* z,
                                                        float* q_out, uint8_t* has_q_out, float* z_out)
{
    const size_t i = blockIdx.x;
    const uint32_t l = lane_id(), ll = l < MOVES ? l : 0;
    bool has_q;
    const float q = root_value(N[i * MOVES + ll], Q[i * MOVES + ll], rfl64(valid[i]), has_q);
    const float zz = blend_z(rdlf(z[i], 0), q, has_q, __fsub_rn(1.0f, q_share), q_share);
    if (l == 0) {
        q_out[i] = q;
        has_q_out[i] = has_q ? 1 : 0;
        z_out[i] = zz;
    }
}

// azr_selfplay_resign_state: each slot's runs, `first` and the holdout coin of its running game (an idle slot: 0, 0, none, not held out)
__global__ __launch_bounds__(64) void k_resign_state(Dev E, uint8_t* run_out, uint8_t* first_out, uint8_t* holdout_out)
{
    const int g = blockIdx.x;
    Ctl c;
    ctl_load(c, &E.ctl[g]);
    const bool on = c.mode != 0;
    const uint32_t rs = on ? rfl(E.resign_state[g]) : 0u;
    if (lane_id() == 0) {
        run_out[2 * g] = (uint8_t)(rs & 255u);
        run_out[2 * g + 1] = (uint8_t)((rs >> 8) & 255u);
        first_out[g] = (uint8_t)resign_first(rs);
        holdout_out[g] = on && resign_holdout(E.resign_threshold, E.resign_seed, c.seed) ? 1 : 0;
    }
}

// azr_debug_resign: the rule alone, one wave per game, through the device functions of the self-play step.  Game i's decisions are rows
// first[i] .. first[i] + game_len[i] - 1 of q / has_q / player.
__global__ __launch_bounds__(64) void k_debug_resign(float q_resign, uint32_t streak, uint32_t threshold, uint32_t seed, const float* q,
                                                     const uint8_t* has_q, const uint8_t* player, const uint32_t* first, const uint32_t* game_len,
                                                     const uint32_t* game_seed, int32_t* row_out, uint8_t* resigner_out, uint8_t* holdout_out)
{
    const size_t i = blockIdx.x;
    const size_t r0 = rfl(first[i]);
    const uint32_t n = rfl(game_len[i]);
    uint32_t rs = 0, who = 255u;
    int32_t row = -1;
    for (uint32_t r = 0; r < n && row < 0; r++) {
        const uint32_t p = rfl((uint32_t)player[r0 + r]) & 1u;
        if (resign_update(rs, p, rdlf(q[r0 + r], 0), rfl((uint32_t)has_q[r0 + r]) != 0u, q_resign, streak)) { row = (int32_t)r; who = p; }
    }
    if (lane_id() == 0) {
        row_out[i] = row;
        resigner_out[i] = (uint8_t)who;
        holdout_out[i] = resign_holdout(threshold, seed, rfl(game_seed[i])) ? 1 : 0;
    }
}

__global__ __launch_bounds__(64) void k_pick(Dev E, int sample, uint8_t* moves)
{
    const int g = blockIdx.x;
    Ctl c;
    ctl_load(c, &E.ctl[g]);
    Tree t = tree_of(E, g);
    WS root;
    ws_load(root, E.state + (size_t)g * GREC);
    root.rng = c.rng;
    uint32_t N; uint64_t valid;
    uint32_t mv = NONE;
    if (root_node(t, root, N, valid) != NO_NODE) {
        float pi = root_policy(N, valid);
        mv = sample ? pick_random(root, pi) : pick_highest(pi);
    }
    if (lane_id() == 0) {
        moves[g] = (uint8_t)mv;
        E.ctl[g].rng = root.rng;
    }
}

// keep != 0: the games go on from the states and RNG streams the caller has set (azr_selfplay_start_from_states)
__global__ __launch_bounds__(64) void k_selfplay_start(Dev E, int keep)
{
    const int g = blockIdx.x;
    Ctl c;
    ctl_load(c, &E.ctl[g]);
    Tree t = tree_of(E, g);
    c.hiwater = (uint32_t)E.C;
    tree_clear(t, c);
    tree_trim(t, c);
    c.mode = 2; c.sims_done = 0; c.sims_started = 0; c.pending = 0; c.search_done = 0; c.error = 0;
    c.game_no = 0; c.nsamples = 0; c.decisions = 0; c.status = ST_NOT_ENDED;
    c.seed = E.base_seed + (uint32_t)g;
    if (E.sp_quota && (unsigned long long)g >= E.sp_quota) c.mode = 0;  // fewer games asked for than slots
    if (!keep) {
        WS s;
        ws_blank(s);
        s.rng = rng_seed(c.seed);
        new_game(s);
        c.rng = s.rng;
        ws_store(s, E.state + (size_t)g * GREC);
    }
    if (lane_id() == 0) E.resign_state[g] = 0u;   // resignation: no run, nobody first (azr_resign.hpp)
    ctl_store(c, &E.ctl[g]);
}

// the first root's vector of every slot (azr_selfplay_start* whose steps carry NOISE).  CAP: a slot whose first decision is fast starts on
// the constant vector; FORCED: so does every root without a draw (no Dirichlet set, or a fast first decision; without a cap the coin says
// full).  Without either the coin is not computed.
template <bool CAP, bool FORCED>
__global__ __launch_bounds__(64) void k_selfplay_noise(Dev E)
{
    const int g = blockIdx.x;
    Ctl c;
    ctl_load(c, &E.ctl[g]);
    WS root;
    ws_load(root, E.state + (size_t)g * GREC);
    new_root_noise<CAP, FORCED>(E, g, c, root, (CAP || FORCED) ? cap_full(E.cap_threshold, E.cap_seed, c.seed, c.decisions) : true);
}

// azr_mcts_pruned_policy: N' and the policy over N' of every game's root, under E.forced_k (<= 0: N' = N) and the root vector in force
// (E.eta_const: none, the constant form)
__global__ __launch_bounds__(64) void k_pruned_policy(Dev E, uint32_t* n_out, float* pi_out)
{
    const int g = blockIdx.x;
    Ctl c;
    ctl_load(c, &E.ctl[g]);
    Tree t = tree_of(E, g);
    WS root;
    ws_load(root, E.state + (size_t)g * GREC);
    const uint32_t l = lane_id();
    const float eta = E.eta_const ? E.noise_value : E.root_eta[(size_t)g * MOVES + (l < MOVES ? l : 0)];
    uint32_t N; uint64_t valid; float pi = 0;
    const uint32_t ridx = root_node(t, root, N, valid);
    if (ridx != NO_NODE) {
        if (E.forced_k > 0.0f) N = root_pruned_counts(E, E.search, t, ridx, N, valid, eta, E.forced_k);
        pi = root_policy(N, valid);
    }
    if (l < MOVES) {
        if (n_out) n_out[(size_t)g * MOVES + l] = N;
        pi_out[(size_t)g * MOVES + l] = pi;
    }
}

// azr_selfplay_decision_kind: the kind of each slot's decision in progress, one wave per game (1 = full, 0 = fast; 1 for an idle slot)
__global__ __launch_bounds__(64) void k_decision_kind(Dev E, uint8_t* out)
{
    const int g = blockIdx.x;
    Ctl c;
    ctl_load(c, &E.ctl[g]);
    const bool full = c.mode == 0 || cap_full(E.cap_threshold, E.cap_seed, c.seed, c.decisions);
    if (lane_id() == 0) out[g] = full ? 1 : 0;
}

// azr_debug_playout_cap: the coin alone, one lane per (game seed, decision)
__global__ __launch_bounds__(64) void k_debug_playout_cap(uint32_t threshold, uint32_t cap_seed, const uint32_t* game_seed, const uint32_t* decision,
                                                          int n, uint8_t* out)
{
    const int i = (int)(blockIdx.x * 64u + threadIdx.x);
    if (i < n) out[i] = cap_full(threshold, cap_seed, game_seed[i], decision[i]) ? 1 : 0;
}

// azr_debug_surprise_weights: the rule alone, one wave per game, through the device functions of the step and its weighted flush.
// Game i's records are rows first[i] .. first[i] + game_len[i] - 1 of pi / prior / valid; its surprises go through kl_out.
__global__ __launch_bounds__(64) void k_debug_surprise(float share, float max_weight, uint32_t seed, const float* pi, const float* prior,
                                                       const uint64_t* valid, const uint32_t* first, const uint32_t* game_len,
                                                       const uint32_t* game_seed, float* kl_out, float* w_out, uint32_t* copies_out)
{
    const size_t i = blockIdx.x;
    const size_t r0 = rfl(first[i]);
    const uint32_t n = rfl(game_len[i]), gs = rfl(game_seed[i]);
    const uint32_t l = lane_id(), ll = l < MOVES ? l : 0;
    for (uint32_t r = 0; r < n; r++) {
        const float kl = record_surprise(pi[(r0 + r) * MOVES + ll], prior[(r0 + r) * MOVES + ll], rfl64(valid[r0 + r]));
        if (l == 0) kl_out[r0 + r] = kl;
    }
    wave_mem_sync();
    const float S = game_surprise_sum(kl_out + r0, n);
    for (uint32_t r = l; r < n; r += 64) {
        const float w = record_weight(kl_out[r0 + r], S, n, share, max_weight);
        w_out[r0 + r] = w;
        copies_out[r0 + r] = record_copies(w, seed, gs, r);
    }
}

// azr_debug_root_noise: the sampler alone, one wave per vector
__global__ __launch_bounds__(64) void k_debug_root_noise(float alpha, uint32_t noise_seed, const uint32_t* game_seed, const uint32_t* decision,
                                                         const uint64_t* valid, float* out)
{
    const size_t i = blockIdx.x;
    const float eta = dirichlet_draw(alpha, noise_seed, rfl(game_seed[i]), rfl(decision[i]), rfl64(valid[i]));
    if (lane_id() < MOVES) out[i * MOVES + lane_id()] = eta;
}

// the first root's g of every slot (azr_selfplay_start* whose steps carry GUMBEL), as k_selfplay_noise is the first root's eta
__global__ __launch_bounds__(64) void k_selfplay_gumbel(Dev E)
{
    const int g = blockIdx.x;
    Ctl c;
    ctl_load(c, &E.ctl[g]);
    WS root;
    ws_load(root, E.state + (size_t)g * GREC);
    new_root_gumbel(E, g, c, root);
}

// the rows of game g's root a Gumbel decision reads (false: the root is not in the tree)
struct GumbelRoot { uint32_t N, N0; float Q, P, g, vhat; uint64_t valid; };
__device__ __forceinline__ bool gumbel_root(const Dev& E, int g, GumbelRoot& r)
{
    Tree t = tree_of(E, g);
    WS root;
    ws_load(root, E.state + (size_t)g * GREC);
    r.Q = r.P = r.g = r.vhat = 0.0f; r.N0 = 0;
    const uint32_t ridx = root_node(t, root, r.N, r.valid, &r.Q, &r.P);
    if (ridx == NO_NODE) return false;
    const uint32_t ll = lane_id() < MOVES ? lane_id() : 0;
    r.N0 = E.root_n0[(size_t)g * MOVES + ll];
    r.g = E.root_g[(size_t)g * MOVES + ll];
    r.vhat = node_vhat(t, ridx);
    return true;
}

// azr_mcts_gumbel_policy: the record's pi and (optional) the completed Q of every game's root, as the self-play decision computes them
__global__ __launch_bounds__(64) void k_gumbel_policy(Dev E, float* qhat_out, float* pi_out)
{
    const int g = blockIdx.x;
    GumbelRoot r;
    float pi = 0.0f, qhat = 0.0f;
    if (gumbel_root(E, g, r)) pi = gumbel_policy(gumbel_score(r.N, r.Q, r.P, r.vhat, r.valid, E.gumbel_cvisit, E.gumbel_cscale), r.valid, &qhat);
    const uint32_t l = lane_id();
    if (l < MOVES) {
        pi_out[(size_t)g * MOVES + l] = pi;
        if (qhat_out) qhat_out[(size_t)g * MOVES + l] = qhat;
    }
}

// azr_mcts_gumbel_pick: the move of every game's decision (NONE for a root that is not in the tree); nothing is drawn
__global__ __launch_bounds__(64) void k_gumbel_pick(Dev E, uint8_t* moves)
{
    const int g = blockIdx.x;
    GumbelRoot r;
    uint32_t mv = NONE;
    if (gumbel_root(E, g, r)) mv = gumbel_move(gumbel_score(r.N, r.Q, r.P, r.vhat, r.valid, E.gumbel_cvisit, E.gumbel_cscale), r.N, r.N0, r.g, r.valid);
    if (lane_id() == 0) moves[g] = (uint8_t)mv;
}

// azr_debug_root_gumbel: the draw alone, one wave per vector
__global__ __launch_bounds__(64) void k_debug_root_gumbel(uint32_t seed, const uint32_t* game_seed, const uint32_t* decision, const uint64_t* valid,
                                                          const uint8_t* greedy, float* out)
{
    const size_t i = blockIdx.x;
    const float gum = gumbel_draw(seed, rfl(game_seed[i]), rfl(decision[i]), rfl64(valid[i]), rfl((uint32_t)greedy[i]) != 0u);
    if (lane_id() < MOVES) out[i * MOVES + lane_id()] = gum;
}

// azr_debug_gumbel_select: the root-level selection alone on synthetic rows, one wave per row
__global__ __launch_bounds__(64) void k_debug_gumbel_select(uint32_t m, uint32_t n, float c_visit, float c_scale, const uint32_t* N, const uint32_t* N0,
                                                            const uint32_t* act, const float* Q, const float* P, const float* g, const float* vhat,
                                                            const uint64_t* valid, const uint32_t* claim, uint8_t* move_out, uint32_t* cv_out)
{
    const size_t i = blockIdx.x;
    const uint32_t l = lane_id(), ll = l < MOVES ? l : 0;
    const size_t at = i * MOVES + ll;
    uint32_t cv;
    const uint32_t W = (N[at] & N_MASK) | (act[at] << 24);
    const uint32_t mv = gumbel_select(W, N0[at], Q[at], P[at], g[at], rdlf(vhat[i], 0), rfl64(valid[i]), rfl(claim[i]), m, n, c_visit, c_scale, cv);
    if (l == 0) {
        move_out[i] = (uint8_t)mv;
        cv_out[i] = cv;
    }
}

// azr_debug_gumbel_tree_select: the selection below the root alone on synthetic rows, one wave per row
__global__ __launch_bounds__(64) void k_debug_gumbel_tree_select(float c_visit, float c_scale, const uint32_t* N, const uint32_t* act, const float* Q,
                                                                 const float* P, const float* vhat, const uint64_t* valid, uint8_t* move_out, float* score_out)
{
    const size_t i = blockIdx.x;
    const uint32_t l = lane_id(), ll = l < MOVES ? l : 0;
    const size_t at = i * MOVES + ll;
    float score;
    const uint32_t W = (N[at] & N_MASK) | (act[at] << 24);
    const uint32_t mv = gumbel_select_tree(W, Q[at], P[at], rdlf(vhat[i], 0), rfl64(valid[i]), c_visit, c_scale, nullptr, nullptr, 0u, &score);
    if (l < MOVES) score_out[at] = score;
    if (l == 0) move_out[i] = (uint8_t)mv;
}

// azr_debug_exp32: the exponential alone, one lane per argument
__global__ __launch_bounds__(64) void k_debug_exp32(const float* x, int n, float* out)
{
    const int i = (int)(blockIdx.x * 64u + threadIdx.x);
    if (i < n) out[i] = exp32(x[i]);
}

// ================================================================================================
// host side
// ================================================================================================
static int next_pow2(int x) { int p = 1; while (p < x) p <<= 1; return p; }

extern "C" void azr_default_settings(azr_settings* s)
{
    memset(s, 0, sizeof *s);
    s->device = 0;
    s->games = 32;
    s->blocks = 20;
    s->net_dtype = AZR_NET_BF16;
    s->mcts_simulations = 32;
    s->mcts_threads = 2;
    s->allow_yield = 1;
    s->limit_reinforcement = 1;
    s->limit_attack = 0;
    s->max_game_rounds = 30 + 28;
    s->min_unit_move = 3;
    s->temperature_threshold = 15 + 28;
    s->hp_exploration = 1.1f;
    s->dir_noise_value = 0.3f;
    s->dir_noise_epsi = 0.25f;
    s->node_capacity = 0;
    s->sample_capacity = 0;
}

template <typename T>
static hipError_t dmalloc(T** p, size_t n) { return hipMalloc((void**)p, n * sizeof(T)); }

static thread_local std::string g_create_err;   // why the last azr_engine_create of this thread failed
static int engine_init(azr_engine* h, const azr_settings* s);

extern "C" int azr_engine_create(const azr_settings* s, azr_engine** out)
{
    if (!out) { g_create_err = "azr_engine_create: out is NULL"; return AZR_E_INVALID_ARGUMENT; }
    *out = nullptr;   // first: every failure below leaves NULL behind and its reason in g_create_err
    auto bad = [&](const std::string& why) { g_create_err = "azr_engine_create: " + why; return (int)AZR_E_INVALID_ARGUMENT; };
    if (!s) return bad("settings is NULL");
    if (s->games <= 0) return bad("games = " + std::to_string(s->games) + " (need > 0)");
    if (s->blocks <= 0) return bad("blocks = " + std::to_string(s->blocks) + " (need > 0)");
    if (s->net_dtype < AZR_NET_F32 || s->net_dtype > AZR_NET_F16) return bad("net_dtype = " + std::to_string(s->net_dtype) + " (AZR_NET_F32 .. AZR_NET_F16)");
    if (s->mcts_simulations < 0) return bad("mcts_simulations = " + std::to_string(s->mcts_simulations) + " (need >= 0)");
    if (s->mcts_threads < 1 || s->mcts_threads > MAX_THREADS)
        return bad("mcts_threads = " + std::to_string(s->mcts_threads) + " (need 1.." + std::to_string(MAX_THREADS) + ")");
    if (s->mcts_simulations > 0 && s->mcts_simulations < s->mcts_threads)   // count = S - S % T would be 0
        return bad("mcts_simulations = " + std::to_string(s->mcts_simulations) + " < mcts_threads = " + std::to_string(s->mcts_threads) +
                   " (S - S % T simulations would be none)");
    // node indices are 16-bit (azr_tree.hpp): a pool above 65 534 nodes per game cannot be addressed.  Rejected, not
    // clamped: a silently smaller pool would change which expansions are dropped.
    const long long want_nodes = s->node_capacity > 0 ? (long long)s->node_capacity : 16ll * (s->mcts_simulations + 1);
    if (want_nodes > 65534) {
        g_create_err = "azr_engine_create: node pool of " + std::to_string(want_nodes) + " nodes per game (node_capacity, or the default "
                       "16 * (mcts_simulations + 1)) exceeds the 65534 a 16-bit node index addresses; pass node_capacity <= 65534";
        return AZR_E_INVALID_ARGUMENT;
    }
    azr_engine* h = new (std::nothrow) azr_engine();
    if (!h) { g_create_err = "azr_engine_create: out of host memory"; return AZR_E_HIP; }
    const int rc_create = engine_init(h, s);
    if (rc_create) {  // nothing half-built is handed out: free what was allocated, keep the message for azr_last_error(NULL)
        g_create_err = h->err;
        azr_engine_destroy(h);
        return rc_create;
    }
    *out = h;
    return AZR_OK;
}

static int engine_init(azr_engine* h, const azr_settings* s)
{
    h->cfg = *s;
    h->mode = 0;
    h->weights_set = false;
    h->prof_net_ms = h->prof_tree_ms = h->prof_tower_ms = 0;
    h->prof_launches = 0;
    h->stream = nullptr;
    Dev& d = h->d;
    memset(&d, 0, sizeof d);
    memset(&h->net, 0, sizeof h->net);
    HIPCHK(h, hipSetDevice(s->device));
    HIPCHK(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    d.G = s->games;
    d.T = s->mcts_threads;
    int C = s->node_capacity > 0 ? s->node_capacity : 16 * (s->mcts_simulations + 1);
    if (C < 8) C = 8;   // H >= 16: one probe round (16 slots) never reads a slot twice
    d.C = C;
    d.H = next_pow2(2 * C);
    d.DMAX = std::min(C, 1024);
#ifdef AZR_TEST_HOOKS
    d.hash_and = hook_env("AZR_TREE_HASH_AND") ? (uint32_t)strtoul(hook_env("AZR_TREE_HASH_AND"), nullptr, 0) : 0xffffffffu;
    d.hash_or = hook_env("AZR_TREE_HASH_OR") ? (uint32_t)strtoul(hook_env("AZR_TREE_HASH_OR"), nullptr, 0) : 0u;
#endif
    d.SCAP = s->sample_capacity > 0 ? s->sample_capacity : 4096;
    d.rules = Rules{s->allow_yield, s->limit_reinforcement, s->limit_attack, s->max_game_rounds, s->min_unit_move};
    // count = MCTS_SIMULATIONS - MCTS_SIMULATIONS % THREADS_PER_MCTS (alphazero_mcts.cpp:265)
    d.search.simulations = s->mcts_simulations - s->mcts_simulations % s->mcts_threads;
    d.search.c1 = 1 - s->dir_noise_epsi;
    d.search.c2 = s->dir_noise_epsi * s->dir_noise_value;
    d.search.hp = s->hp_exploration;
    d.search.temperature_threshold = s->temperature_threshold;
    d.noise_eps = s->dir_noise_epsi;
    d.noise_value = s->dir_noise_value;
    d.cap_threshold = 1u << 24;   // no cap: every decision is full
    d.cap_seed = 0;
    d.cap_fast = d.search.simulations;
    d.forced_k = 0.0f;            // no forced playouts, no pruning
    d.prune = 0;
    d.eta_const = 0;
    d.search2_simulations = d.search.simulations;   // player B of a two-net arena: this handle's own until azr_arena_set_opponent_search
    d.search2_hp = d.search.hp;
    const size_t G = d.G, GT = G * d.T;
    HIPCHK(h, dmalloc(&d.state, G * GREC));
    HIPCHK(h, dmalloc(&d.ctl, G));
    HIPCHK(h, dmalloc(&d.nodes, G * C * NODE_BYTES));
    HIPCHK(h, dmalloc(&d.touch, G * C));
    HIPCHK(h, dmalloc(&d.nhash, G * C));
    HIPCHK(h, dmalloc(&d.table, G * d.H));
    HIPCHK(h, dmalloc(&d.freel, G * C));
    HIPCHK(h, dmalloc(&d.path, GT * d.DMAX));
    HIPCHK(h, dmalloc(&d.leaf_in, GT * LEAF_STRIDE));
    HIPCHK(h, dmalloc(&d.leaf_key, GT * GREC));
    HIPCHK(h, dmalloc(&d.leaf_valid, GT));
    HIPCHK(h, dmalloc(&d.leaf_hash, GT));
    HIPCHK(h, dmalloc(&d.net_pi, GT * PI_STRIDE));
    HIPCHK(h, dmalloc(&d.net_v, GT));
    HIPCHK(h, dmalloc(&d.stage, G * d.SCAP * STAGE_BYTES));
    d.ring_cap = (unsigned long long)G * d.SCAP;
    HIPCHK(h, dmalloc(&d.ring, (size_t)d.ring_cap * AZR_RECORD_BYTES));
    HIPCHK(h, dmalloc(&d.ring_count, 2));   // [0] records in the ring, [1] ring room claimed by scripted collection (ring_reserve)
    HIPCHK(h, dmalloc(&d.counters, G));   // one row per game
    HIPCHK(h, dmalloc(&d.active, 1));
    HIPCHK(h, dmalloc(&d.arena_taken, 1));
    HIPCHK(h, dmalloc(&d.sp_started, 1));
    HIPCHK(h, dmalloc(&d.leaf_list, 2 * GT));      // leaf slots waiting for net A / net B (two-net arena; self-play tail uses [0])
    HIPCHK(h, dmalloc(&d.leaf_count, (size_t)4));
    d.lc_base = 0; d.lc_zero = -1;
    HIPCHK(h, dmalloc(&d.arena_res, 8));
    HIPCHK(h, dmalloc(&d.prev_start, G * GREC));
    HIPCHK(h, dmalloc(&d.script, G * 2 * 32));
    HIPCHK(h, dmalloc(&d.alog_status, G * ALOG));
    HIPCHK(h, dmalloc(&d.alog_rounds, G * ALOG));
    HIPCHK(h, dmalloc(&d.alog_final, G * ALOG * GREC));
    HIPCHK(h, dmalloc(&d.root_eta, G * MOVES));
    HIPCHK(h, dmalloc(&d.resign_state, G));
    HIPCHK(h, dmalloc(&d.resign_stats, G * 4));
    HIPCHK(h, hipMemsetAsync(d.root_eta, 0, G * MOVES * sizeof(float), h->stream));
    HIPCHK(h, hipMemsetAsync(d.state, 0, G * GREC, h->stream));
    HIPCHK(h, hipMemsetAsync(d.ctl, 0, G * sizeof(Ctl), h->stream));
    HIPCHK(h, hipMemsetAsync(d.touch, 0, G * C * sizeof(uint32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(d.table, 0, G * d.H * sizeof(uint32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(d.leaf_in, 0, GT * LEAF_STRIDE, h->stream));
    HIPCHK(h, hipMemsetAsync(d.net_pi, 0, GT * PI_STRIDE * sizeof(float), h->stream));
    HIPCHK(h, hipMemsetAsync(d.net_v, 0, GT * sizeof(float), h->stream));
    HIPCHK(h, hipMemsetAsync(d.ring_count, 0, 2 * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(d.counters, 0, (size_t)d.G * sizeof(Counters), h->stream));
    HIPCHK(h, hipMemsetAsync(d.resign_state, 0, G * sizeof(uint32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(d.resign_stats, 0, G * 4 * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(d.active, 0, sizeof(uint32_t), h->stream));
    int rc = net_alloc(h);
    if (rc) return rc;
    hipLaunchKernelGGL(k_tree_clear, dim3(d.G), dim3(64), 0, h->stream, d);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return AZR_OK;
}

extern "C" int azr_engine_destroy(azr_engine* h)
{
    if (!h) return AZR_E_BAD_HANDLE;
    hipSetDevice(h->cfg.device);
    if (h->stream) hipStreamSynchronize(h->stream);
    Dev& d = h->d;
    void* ptrs[] = {d.sp_started, d.state, d.ctl, d.nodes, d.touch, d.nhash, d.table, d.freel, d.path, d.leaf_in, d.leaf_key,
                    d.leaf_valid, d.leaf_hash, d.net_pi, d.net_v, d.stage, d.ring, d.ring_count, d.counters, d.active,
                    d.arena_taken, d.arena_res, d.prev_start, d.script, d.alog_status, d.alog_rounds, d.alog_final, d.root_eta, d.stage_kl,
                    d.stage_q, d.resign_state, d.resign_stats, d.root_g, d.root_n0};
    for (void* p : ptrs) if (p) hipFree(p);
    for (void* p : h->tree2) if (p) hipFree(p);
    if (d.leaf_list) hipFree(d.leaf_list);
    if (d.leaf_count) hipFree(d.leaf_count);
    dp_free(h);
    train_free(h);
    net_free(h);
    for (const ProfEvents& e : h->ev)
        for (hipEvent_t x : {e.tree0, e.tree1, e.net1, e.tower0, e.tower1}) if (x) hipEventDestroy(x);
#ifdef AZR_TREE_PROF
    {
        unsigned long long t[25] = {0}, u[25] = {0}, hh[16] = {0};
        (void)hipMemcpyFromSymbol(t, HIP_SYMBOL(azr::g_tprof), sizeof t);
        (void)hipMemcpyFromSymbol(u, HIP_SYMBOL(azr::g_tslow), sizeof u);
        (void)hipMemcpyFromSymbol(hh, HIP_SYMBOL(azr::g_thist), sizeof hh);
        static const char* nm[24] = {"prologue", "consume: read leaf", "consume: dup lookup", "consume: normalize", "consume: expand", "backup",
                                     "loop/copy root", "game_status", "valid_moves", "record+hash", "lookup", "leaf write", "select", "make_move", "decision: trim", "epilogue: leaf list",
                                     "decision: policy+pick+stage", "decision: make_move+status", "decision: flush+next game", "epilogue: ws_store", "epilogue: ctl_store", "epilogue: counters", "make_move: fortify", "make_move: attack"};
        if (t[24]) {
            fprintf(stderr, "tree step profile: %llu waves, us per wave:", t[24]); double sum = 0;
            for (int i = 0; i < 24; i++) { fprintf(stderr, " %s %.2f |", nm[i], t[i] * 0.01 / t[24]); sum += t[i] * 0.01 / t[24]; } fprintf(stderr, " total %.2f\n", sum);
            if (u[24]) { fprintf(stderr, "  waves over 60 us: %llu, us per wave:", u[24]); for (int i = 0; i < 24; i++) fprintf(stderr, " %s %.2f |", nm[i], u[i] * 0.01 / u[24]); fprintf(stderr, "\n"); }
            fprintf(stderr, "  waves by total time, 10-us bins:"); for (int i = 0; i < 16; i++) fprintf(stderr, " %llu", hh[i]); fprintf(stderr, "\n");
            unsigned long long z[25] = {0};
            (void)hipMemcpyToSymbol(HIP_SYMBOL(azr::g_tprof), z, sizeof z); (void)hipMemcpyToSymbol(HIP_SYMBOL(azr::g_tslow), z, sizeof z); (void)hipMemcpyToSymbol(HIP_SYMBOL(azr::g_thist), z, sizeof(unsigned long long) * 16);
        }
    }
#endif
    if (h->arena_ev) hipEventDestroy(h->arena_ev);
    if (h->arena_ev2) hipEventDestroy(h->arena_ev2);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
    return AZR_OK;
}

extern "C" const char* azr_last_error(const azr_engine* h)
{
    if (h) return h->err.c_str();
    return g_create_err.empty() ? "bad handle" : g_create_err.c_str();   // NULL: the calling thread's last failed create
}
extern "C" int azr_engine_games(const azr_engine* h) { return h ? h->d.G : 0; }

// staging helpers: synchronous copies through temporary device buffers (boundary calls are not the hot path)
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(&p, n ? n : 1); }
};
#define H2D(h, dst, src, n) HIPCHK(h, hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, (h)->stream))
#define D2H(h, dst, src, n) HIPCHK(h, hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, (h)->stream))
#define SYNC(h) HIPCHK(h, hipStreamSynchronize((h)->stream))
#define LAUNCH(h, kern, ...)                                                          \
    do {                                                                              \
        hipLaunchKernelGGL(kern, dim3((h)->d.G), dim3(64), 0, (h)->stream, __VA_ARGS__); \
        HIPCHK(h, hipGetLastError());                                                 \
    } while (0)
// the arena step of this handle: with a Gumbel side (azr_arena_set_gumbel), with the scripted players' recorder
// (azr_arena_collect_scripted_samples) or without either; azr_arena_start refuses the first two together
#define ARENA_STEP(h, dev)                                                                  \
    do {                                                                                    \
        if ((h)->arena_gumbel) LAUNCH(h, k_arena_step_gumbel, dev, (h)->arena_gumbel_run);  \
        else LAUNCH(h, (h)->arena_rec ? k_arena_step_rec : k_arena_step, dev);              \
    } while (0)
// a boundary call that hands back one array: `kern(args..., buf)` fills a temporary device buffer of `bytes`, copied out to `dst`
#define LAUNCH_OUT(h, dst, bytes, T, kern, ...)              \
    do {                                                     \
        DevBuf buf_;                                          \
        HIPCHK(h, buf_.alloc(bytes));                         \
        LAUNCH(h, kern, __VA_ARGS__, (T*)buf_.p);             \
        D2H(h, dst, buf_.p, bytes);                           \
        SYNC(h);                                             \
    } while (0)
#define ENTER(h)                                 \
    if (!(h)) return AZR_E_BAD_HANDLE;           \
    HIPCHK(h, hipSetDevice((h)->cfg.device))

static int bad_argument(azr_engine* h, const std::string& why) { h->err = why; return AZR_E_INVALID_ARGUMENT; }

// The staging of a boundary call around one launch.  in(): a device copy of a host array of n elements.  out(): a device buffer of n
// elements that goes back to a host array after the launch (no host array: an output nobody asked for; the kernel still gets its
// buffer).  The first HIP error is kept and makes the calls behind it return nullptr; STAGED_LAUNCH hands it to HIPCHK before anything
// is launched.  Every buffer is freed when the struct goes.
struct Stage {
    struct Buf { void* dev; void* host; size_t bytes; };
    azr_engine* h;
    hipError_t err = hipSuccess;
    std::vector<Buf> bufs;
    explicit Stage(azr_engine* h_) : h(h_) {}
    ~Stage() { for (Buf& b : bufs) hipFree(b.dev); }
    void* buf(const void* src, void* dst, size_t bytes)
    {
        void* p = nullptr;
        if (err == hipSuccess) err = hipMalloc(&p, bytes ? bytes : 1);
        if (err != hipSuccess) return nullptr;
        bufs.push_back({p, dst, bytes});
        if (src && bytes) err = hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, h->stream);
        return p;
    }
    template <class T> const T* in(const T* src, size_t n) { return (const T*)buf(src, nullptr, n * sizeof(T)); }
    template <class T> T* out(T* dst, size_t n) { return (T*)buf(nullptr, dst, n * sizeof(T)); }
    hipError_t finish()   // behind the launch: its error, every output that was asked for, the stream drained
    {
        err = hipGetLastError();
        for (Buf& b : bufs)
            if (err == hipSuccess && b.host) err = hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, h->stream);
        return err == hipSuccess ? hipStreamSynchronize(h->stream) : err;
    }
};
#define STAGED_LAUNCH(st, kern, blocks, ...)                                                      \
    do {                                                                                          \
        HIPCHK((st).h, (st).err);                                                                 \
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(64), 0, (st).h->stream, __VA_ARGS__);         \
        HIPCHK((st).h, (st).finish());                                                            \
    } while (0)

// the first row of each game where the games' rows lie one behind the other; false where they are more than 2^31 - 1
static bool first_rows(const uint32_t* game_len, int games, std::vector<uint32_t>& first, size_t& rows)
{
    first.resize((size_t)games);
    rows = 0;
    for (int i = 0; i < games; i++) {
        first[i] = (uint32_t)rows;
        rows += game_len[i];
        if (rows > 0x7fffffffu) return false;
    }
    return true;
}

// one 32-bit field of every game's Ctl line <-> a packed host array of G values (`field` = offsetof(Ctl, ...)): a strided copy queued on
// the handle's stream, the caller synchronises
static hipError_t ctl_field_get(azr_engine* h, size_t field, void* dst)
{
    return hipMemcpy2DAsync(dst, 4, (const uint8_t*)h->d.ctl + field, sizeof(Ctl), 4, h->d.G, hipMemcpyDeviceToHost, h->stream);
}
static hipError_t ctl_field_set(azr_engine* h, size_t field, const void* src)
{
    return hipMemcpy2DAsync((uint8_t*)h->d.ctl + field, sizeof(Ctl), src, 4, 4, h->d.G, hipMemcpyHostToDevice, h->stream);
}

extern "C" int azr_engine_new_games(azr_engine* h, const uint32_t* seeds)
{
    ENTER(h);
    if (!seeds) return AZR_E_INVALID_ARGUMENT;
    DevBuf b;
    HIPCHK(h, b.alloc(h->d.G * 4));
    H2D(h, b.p, seeds, (size_t)h->d.G * 4);
    LAUNCH(h, k_new_games, h->d, (const uint32_t*)b.p);
    LAUNCH(h, k_tree_clear, h->d);
    SYNC(h);
    return AZR_OK;
}

extern "C" int azr_engine_set_states(azr_engine* h, const void* data160)
{
    ENTER(h);
    if (!data160) return AZR_E_INVALID_ARGUMENT;
    DevBuf b;
    HIPCHK(h, b.alloc((size_t)h->d.G * 160));
    H2D(h, b.p, data160, (size_t)h->d.G * 160);
    LAUNCH(h, k_import160, h->d, (const uint8_t*)b.p);
    SYNC(h);
    return AZR_OK;
}

extern "C" int azr_engine_get_states(azr_engine* h, void* data160)
{
    ENTER(h);
    if (!data160) return AZR_E_INVALID_ARGUMENT;
    LAUNCH_OUT(h, data160, (size_t)h->d.G * 160, uint8_t, k_export160, h->d, (const uint8_t*)h->d.state);
    return AZR_OK;
}

extern "C" int azr_engine_set_rng(azr_engine* h, const uint32_t* st)
{
    ENTER(h);
    if (!st) return AZR_E_INVALID_ARGUMENT;
    HIPCHK(h, ctl_field_set(h, offsetof(Ctl, rng), st));
    SYNC(h);
    return AZR_OK;
}

extern "C" int azr_engine_get_rng(azr_engine* h, uint32_t* st)
{
    ENTER(h);
    if (!st) return AZR_E_INVALID_ARGUMENT;
    HIPCHK(h, ctl_field_get(h, offsetof(Ctl, rng), st));
    SYNC(h);
    return AZR_OK;
}

extern "C" int azr_engine_valid_moves(azr_engine* h, uint64_t* masks)
{
    ENTER(h);
    if (!masks) return AZR_E_INVALID_ARGUMENT;
    LAUNCH_OUT(h, masks, (size_t)h->d.G * 8, uint64_t, k_valid_moves, h->d);
    return AZR_OK;
}

extern "C" int azr_engine_make_moves(azr_engine* h, const uint8_t* moves, uint8_t* rc)
{
    ENTER(h);
    if (!moves) return AZR_E_INVALID_ARGUMENT;
    DevBuf b, r;
    HIPCHK(h, b.alloc(h->d.G));
    HIPCHK(h, r.alloc(h->d.G));
    H2D(h, b.p, moves, (size_t)h->d.G);
    LAUNCH(h, k_make_moves, h->d, (const uint8_t*)b.p, (uint8_t*)r.p);
    std::vector<uint8_t> tmp(h->d.G);
    D2H(h, tmp.data(), r.p, (size_t)h->d.G);
    SYNC(h);
    int worst = AZR_OK;
    for (int g = 0; g < h->d.G; g++) {
        if (rc) rc[g] = tmp[g];
        if (tmp[g] && !worst) worst = tmp[g];
    }
    return rc ? AZR_OK : worst;
}

extern "C" int azr_engine_status(azr_engine* h, int8_t* status)
{
    ENTER(h);
    if (!status) return AZR_E_INVALID_ARGUMENT;
    LAUNCH_OUT(h, status, (size_t)h->d.G, int8_t, k_status, h->d);
    return AZR_OK;
}

extern "C" int azr_engine_encode(azr_engine* h, void* in88)
{
    ENTER(h);
    if (!in88) return AZR_E_INVALID_ARGUMENT;
    DevBuf b;
    HIPCHK(h, b.alloc((size_t)h->d.G * 88));
    HIPCHK(h, hipMemsetAsync(b.p, 0, (size_t)h->d.G * 88, h->stream));
    LAUNCH(h, k_encode, h->d, (uint8_t*)b.p);
    D2H(h, in88, b.p, (size_t)h->d.G * 88);
    SYNC(h);
    return AZR_OK;
}

// ---- search ---------------------------------------------------------------------------------------
extern "C" int azr_mcts_clear(azr_engine* h)
{
    ENTER(h);
    LAUNCH(h, k_tree_clear, h->d);
    SYNC(h);
    return AZR_OK;
}

extern "C" int azr_mcts_trim(azr_engine* h)
{
    ENTER(h);
    LAUNCH(h, k_tree_trim, h->d);
    SYNC(h);
    return AZR_OK;
}

extern "C" int azr_mcts_begin(azr_engine* h)
{
    ENTER(h);
    // a Gumbel search after an arena: the arena's steps expanded nodes without the net's value, and none of them may be searched
    if (h->mode == 3 && h->host.gumbel_m > 0) LAUNCH(h, k_tree_clear, h->d);
    h->mode = 1;
    LAUNCH(h, k_search_begin, h->d);
    SYNC(h);
    return AZR_OK;
}

// The thirty-seven k_tree_step instantiations, named here only: host-stepped or self-play, each plain, with NOISE and with NOISE + FORCED;
// self-play also under a CAP, which doubles its three, each of those six with SURPRISE, and each of those twelve with QMIX; the five
// with GUMBEL: host-stepped, and self-play with and without SURPRISE and QMIX; and those five again with GTREE.  CAP, SURPRISE and QMIX
// need SELFPLAY, FORCED implies NOISE, GUMBEL excludes NOISE, CAP and FORCED, GTREE needs GUMBEL (k_tree_step asserts all six).
// Callers say what is in force; forced playouts without root noise run the NOISE instantiation, on the constant vector.
static int launch_tree_step(azr_engine* h, const Dev& d, bool selfplay, const StepOpts& o)
{
    void (*step)(Dev) = nullptr;
#define AZR_STEP(SP, N, C, F, W, M) \
    case (M) << 5 | (W) << 4 | (SP) << 3 | (N) << 2 | (C) << 1 | (F): step = k_tree_step<SP, N, C, F, W, M>; break
#define AZR_STEP_GUMBEL(SP, W, M, GT) \
    case (GT) << 7 | 1 << 6 | (M) << 5 | (W) << 4 | (SP) << 3: step = k_tree_step<SP, 0, 0, 0, W, M, 1, GT>; break
#define AZR_STEP_SP(W, M) \
    AZR_STEP(1, 0, 0, 0, W, M); AZR_STEP(1, 1, 0, 0, W, M); AZR_STEP(1, 1, 0, 1, W, M); \
    AZR_STEP(1, 0, 1, 0, W, M); AZR_STEP(1, 1, 1, 0, W, M); AZR_STEP(1, 1, 1, 1, W, M)
    // (the fifteen without QMIX first, in the order they always had, then their self-play twelve again with QMIX)
    switch (o.gtree << 7 | o.gumbel << 6 | o.qmix << 5 | o.surprise << 4 | selfplay << 3 | (o.noise || o.forced) << 2 | o.cap << 1 | o.forced) {
        AZR_STEP(0, 0, 0, 0, 0, 0); AZR_STEP(0, 1, 0, 0, 0, 0); AZR_STEP(0, 1, 0, 1, 0, 0);
        AZR_STEP_SP(0, 0);
        AZR_STEP_SP(1, 0);
        AZR_STEP_SP(0, 1);
        AZR_STEP_SP(1, 1);
        AZR_STEP_GUMBEL(0, 0, 0, 0);
        AZR_STEP_GUMBEL(1, 0, 0, 0); AZR_STEP_GUMBEL(1, 1, 0, 0); AZR_STEP_GUMBEL(1, 0, 1, 0); AZR_STEP_GUMBEL(1, 1, 1, 0);
        AZR_STEP_GUMBEL(0, 0, 0, 1);
        AZR_STEP_GUMBEL(1, 0, 0, 1); AZR_STEP_GUMBEL(1, 1, 0, 1); AZR_STEP_GUMBEL(1, 0, 1, 1); AZR_STEP_GUMBEL(1, 1, 1, 1);
    }
#undef AZR_STEP_GUMBEL
#undef AZR_STEP_SP
#undef AZR_STEP
    if (!step) {
        h->err = "launch_tree_step: a playout cap, surprise weighting or a value mix on a host-stepped search, a Gumbel search with root "
                 "noise, a playout cap or forced playouts, or the Gumbel selection below the root without a Gumbel search: there is no such k_tree_step";
        return AZR_E_LOGIC;
    }
    hipLaunchKernelGGL(step, dim3(d.G), dim3(64), 0, h->stream, d);
    HIPCHK(h, hipGetLastError());
    return AZR_OK;
}

// What is in force in `mode` (the handle's, or 1 for a host-stepped step whatever the handle ran before): a running self-play's options
// as azr_selfplay_start* found them, nothing in an arena, else the host-stepped ones as they stand.
static StepOpts options_in_force(const azr_engine* h, int mode)
{
    if (mode == 2) return h->sp;
    if (mode == 3) return StepOpts{};
    return StepOpts{h->host.noise, false, h->host.forced_k > 0.0f, false, false, h->host.gumbel_m > 0, h->host.gumbel_m > 0 && h->host.gumbel_tree};
}
// ... and the device view a search-related launch sees with it.  eta_const: no root vector is there to read (a self-play whose steps
// carry NOISE keeps one per root).  Outside a self-play: the handle's without a self-play's leftovers, with azr_mcts_set_forced_playouts /
// azr_mcts_set_simulations / azr_mcts_set_gumbel applied; the steps without FORCED read none of forced_k, prune and eta_const, the steps
// without GUMBEL none of gumbel_*.
static Dev search_view(const azr_engine* h, int mode)
{
    Dev d = h->d;
    const StepOpts o = options_in_force(h, mode);
    d.eta_const = (o.noise || (mode == 2 && o.forced)) ? 0 : 1;
    if (mode == 2) return d;
    d.forced_k = o.forced ? h->host.forced_k : 0.0f;
    d.prune = 0;
    d.gumbel_m = mode != 3 ? h->host.gumbel_m : 0;
    d.gumbel_cvisit = h->host.gumbel_cvisit;
    d.gumbel_cscale = h->host.gumbel_cscale;
    if (mode != 3 && h->host.sims > 0) d.search.simulations = h->host.sims - h->host.sims % d.T;
    return d;
}

static int tree_step_host(azr_engine* h, uint32_t* active)
{
    HIPCHK(h, hipMemsetAsync(h->d.active, 0, 4, h->stream));
    if (int rc = launch_tree_step(h, search_view(h, 1), false, options_in_force(h, 1))) return rc;
    D2H(h, active, h->d.active, 4);
    SYNC(h);
    return AZR_OK;
}

extern "C" int azr_mcts_leaves(azr_engine* h, void* in88, uint8_t* need, int* active_out)
{
    ENTER(h);
    uint32_t active = 0;
    int rc = tree_step_host(h, &active);
    if (rc) return rc;
    const int G = h->d.G, T = h->d.T;
    if (in88) HIPCHK(h, hipMemcpy2DAsync(in88, 88, h->d.leaf_in, LEAF_STRIDE, 88, (size_t)G * T, hipMemcpyDeviceToHost, h->stream));
    if (need) {
        std::vector<uint32_t> p(G);
        HIPCHK(h, ctl_field_get(h, offsetof(Ctl, pending), p.data()));
        SYNC(h);
        for (int g = 0; g < G; g++)
            for (int k = 0; k < T; k++) need[g * T + k] = (uint8_t)((p[g] >> k) & 1u);
    }
    SYNC(h);
    if (active_out) *active_out = (int)active;
    return AZR_OK;
}

extern "C" int azr_mcts_apply(azr_engine* h, const float* pi, const float* v)
{
    ENTER(h);
    if (!pi || !v) return AZR_E_INVALID_ARGUMENT;
    const size_t GT = (size_t)h->d.G * h->d.T;
    HIPCHK(h, hipMemcpy2DAsync(h->d.net_pi, PI_STRIDE * 4, pi, MOVES * 4, MOVES * 4, GT, hipMemcpyHostToDevice, h->stream));
    H2D(h, h->d.net_v, v, GT * 4);
    SYNC(h);
    return AZR_OK;
}

extern "C" int azr_mcts_simulate(azr_engine* h)
{
    ENTER(h);
    if (!h->weights_set) { h->err = "azr_mcts_simulate: no weights (azr_nn_init_random / azr_nn_set_weights / azr_nn_load)"; return AZR_E_STATE; }
    int rc = azr_mcts_begin(h);
    if (rc) return rc;
    for (;;) {
        uint32_t active = 0;
        rc = tree_step_host(h, &active);
        if (rc) return rc;
        if (active == 0) break;
        rc = net_forward(h, h->d.leaf_in, LEAF_STRIDE, h->d.G * h->d.T, h->d.net_pi, h->d.net_v);
        if (rc) return rc;
    }
    // surface per-game errors
    std::vector<uint32_t> e(h->d.G);
    HIPCHK(h, ctl_field_get(h, offsetof(Ctl, error), e.data()));
    SYNC(h);
    for (int g = 0; g < h->d.G; g++)
        if (e[g]) { h->err = "search error in game " + std::to_string(g) + " code " + std::to_string(e[g]); return (int)e[g]; }
    return AZR_OK;
}

extern "C" int azr_mcts_root_stats(azr_engine* h, uint32_t* n, float* q, float* p)
{
    ENTER(h);
    const size_t sz = (size_t)h->d.G * MOVES;
    Stage st(h);
    uint32_t* dn = st.out(n, sz);
    float *dq = st.out(q, sz), *dp = st.out(p, sz);
    STAGED_LAUNCH(st, k_root_stats, h->d.G, h->d, dn, dq, dp, (float*)nullptr);
    return AZR_OK;
}

extern "C" int azr_mcts_node_stats(azr_engine* h, const void* data160, uint32_t* n, uint32_t* act, float* q, float* p, float* vhat, uint8_t* found)
{
    ENTER(h);
    if (!data160 || !n || !q || !p || !found) return AZR_E_INVALID_ARGUMENT;
    const size_t G = (size_t)h->d.G, sz = G * MOVES;
    Stage st(h);
    const uint8_t* dd = st.in((const uint8_t*)data160, G * 160);
    uint32_t *dn = st.out(n, sz), *da = act ? st.out(act, sz) : nullptr;
    float *dq = st.out(q, sz), *dp = st.out(p, sz), *dv = vhat ? st.out(vhat, G) : nullptr;
    uint8_t* df = st.out(found, G);
    STAGED_LAUNCH(st, k_node_stats, h->d.G, h->d, dd, dn, da, dq, dp, dv, df);
    return AZR_OK;
}

extern "C" int azr_mcts_root_value(azr_engine* h, float* q, uint8_t* has_q)
{
    ENTER(h);
    if (!q) return AZR_E_INVALID_ARGUMENT;
    Stage st(h);
    float* dq = st.out(q, (size_t)h->d.G);
    uint8_t* dh = st.out(has_q, (size_t)h->d.G);
    STAGED_LAUNCH(st, k_root_value, h->d.G, h->d, dq, dh);
    return AZR_OK;
}

extern "C" int azr_mcts_policy(azr_engine* h, float* pi)
{
    ENTER(h);
    if (!pi) return AZR_E_INVALID_ARGUMENT;
    LAUNCH_OUT(h, pi, (size_t)h->d.G * MOVES * 4, float, k_root_stats, h->d, (uint32_t*)nullptr, (float*)nullptr, (float*)nullptr);
    return AZR_OK;
}

extern "C" int azr_mcts_pick(azr_engine* h, int sample, uint8_t* moves)
{
    ENTER(h);
    if (!moves) return AZR_E_INVALID_ARGUMENT;
    LAUNCH_OUT(h, moves, (size_t)h->d.G, uint8_t, k_pick, h->d, sample);
    return AZR_OK;
}

// ---- device-resident self-play ------------------------------------------------------------------------
// a playout cap's full_prob: a number >= 0, and the coin's threshold it stands for (2^24, every decision full, from 1 up)
static int full_prob_check(azr_engine* h, const char* who, float full_prob, const char* note)
{
    return full_prob >= 0.0f ? AZR_OK : bad_argument(h, std::string(who) + ": full_prob must be a number >= 0" + note);   // (NaN fails)
}
static uint32_t cap_threshold_of(float full_prob) { return full_prob >= 1.0f ? (1u << 24) : (uint32_t)(full_prob * 16777216.0f); }
// the holdout coin's threshold of a resignation's holdout_share in [0, 1] (2^24 at 1: every game is held out)
static uint32_t resign_threshold_of(float holdout_share) { return (uint32_t)(holdout_share * 16777216.0f); }

// The azr_selfplay_set_* options as they stand now, into what this self-play's steps carry (h->sp) and the Dev fields they read: a
// running self-play never sees a setter's change.  The host-stepped options end here (root_eta is this self-play's from now on).
static void resolve_selfplay_options(azr_engine* h)
{
    const SelfplayOpts& o = h->sp_set;
    Dev& d = h->d;
    h->host = HostOpts{};
    h->sp = StepOpts{o.alpha > 0.0f, o.cap_prob < 1.0f && o.cap_fast_sims > 0, o.forced_k > 0.0f, o.psw_share > 0.0f, o.q_share > 0.0f, o.gumbel_m > 0, o.gumbel_m > 0 && o.gumbel_tree != 0};
    d.noise_alpha = o.alpha;
    d.noise_seed = o.noise_seed;
    d.cap_threshold = cap_threshold_of(o.cap_prob);
    d.cap_seed = o.cap_seed;
    d.cap_fast = h->sp.cap ? o.cap_fast_sims - o.cap_fast_sims % d.T : d.search.simulations;
    d.forced_k = o.forced_k;
    d.prune = h->sp.forced && o.prune ? 1 : 0;
    d.psw_share = o.psw_share;
    d.psw_max = o.psw_max;
    d.psw_seed = o.psw_seed;
    d.q_share = o.q_share;
    d.resign_streak = o.resign_streak;
    d.resign_q = o.resign_q;
    d.resign_threshold = resign_threshold_of(o.resign_holdout);
    d.resign_seed = o.resign_seed;
    d.gumbel_m = o.gumbel_m;
    d.gumbel_cvisit = o.gumbel_cvisit;
    d.gumbel_cscale = o.gumbel_cscale;
    d.gumbel_seed = o.gumbel_seed;
    d.eta_const = 0;
}

// the Gumbel search's two per-game rows, with the first search that needs them: an engine that never runs one allocates none.  The N0
// rows alone serve an arena with a Gumbel side, whose g is 0.
static int gumbel_alloc_n0(azr_engine* h)
{
    const size_t n = (size_t)h->d.G * MOVES;
    if (!h->d.root_n0) {
        HIPCHK(h, dmalloc(&h->d.root_n0, n));
        HIPCHK(h, hipMemsetAsync(h->d.root_n0, 0, n * sizeof(uint32_t), h->stream));
    }
    return AZR_OK;
}
static int gumbel_alloc(azr_engine* h)
{
    const size_t n = (size_t)h->d.G * MOVES;
    if (!h->d.root_g) {
        HIPCHK(h, dmalloc(&h->d.root_g, n));
        HIPCHK(h, hipMemsetAsync(h->d.root_g, 0, n * sizeof(float), h->stream));
    }
    return gumbel_alloc_n0(h);
}

static int selfplay_start(azr_engine* h, uint32_t base_seed, unsigned long long quota, int keep = 0)
{
    // a Gumbel search has no root noise, no fast decisions and no forced playouts: refused before anything of the handle changes
    if (h->sp_set.gumbel_m > 0) {
        const SelfplayOpts& o = h->sp_set;
        const char* other = o.alpha > 0.0f ? "Dirichlet noise (azr_selfplay_set_dirichlet)" :
                            (o.cap_prob < 1.0f && o.cap_fast_sims > 0) ? "a playout cap (azr_selfplay_set_playout_cap)" :
                            o.forced_k > 0.0f ? "forced playouts (azr_selfplay_set_forced_playouts)" : nullptr;
        if (other) return bad_argument(h, std::string("azr_selfplay_start: the Gumbel root search (azr_selfplay_set_gumbel) does not go with ") + other + ": switch one of them off");
        if (int rc = gumbel_alloc(h)) return rc;
    } else if (h->sp_set.gumbel_tree)
        return bad_argument(h, "azr_selfplay_start: the Gumbel selection below the root (azr_selfplay_set_gumbel_tree) needs the Gumbel root search "
                               "(azr_selfplay_set_gumbel with m > 0): switch the one off or the other on");
    // the surprises' buffer, with the first self-play that weights its records: an engine that never does allocates none
    if (h->sp_set.psw_share > 0.0f && !h->d.stage_kl) HIPCHK(h, dmalloc(&h->d.stage_kl, (size_t)h->d.G * h->d.SCAP));
    // ... and the root values' buffer, with the first self-play that blends them into z
    if (h->sp_set.q_share > 0.0f && !h->d.stage_q) HIPCHK(h, dmalloc(&h->d.stage_q, (size_t)h->d.G * h->d.SCAP));
    h->d.base_seed = base_seed;
    h->d.sp_quota = quota;
    h->d.sp_compact = 0;
    h->sp_tail = false;
    h->mode = 2;
    const unsigned long long started = quota ? std::min<unsigned long long>(quota, (unsigned long long)h->d.G) : 0ull;
    HIPCHK(h, hipMemcpyAsync(h->d.sp_started, &started, sizeof started, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(h->d.counters, 0, (size_t)h->d.G * sizeof(Counters), h->stream));
    HIPCHK(h, hipMemsetAsync(h->d.resign_stats, 0, (size_t)h->d.G * 4 * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(h->d.ring_count, 0, sizeof(unsigned long long), h->stream));
    LAUNCH(h, k_selfplay_start, h->d, keep);
    resolve_selfplay_options(h);
    if (h->sp.forced) LAUNCH(h, (k_selfplay_noise<false, true>), h->d);
    else if (h->sp.noise && h->sp.cap) LAUNCH(h, (k_selfplay_noise<true, false>), h->d);
    else if (h->sp.noise) LAUNCH(h, (k_selfplay_noise<false, false>), h->d);
    else HIPCHK(h, hipMemsetAsync(h->d.root_eta, 0, (size_t)h->d.G * MOVES * sizeof(float), h->stream));
    if (h->sp.gumbel) LAUNCH(h, k_selfplay_gumbel, h->d);
    SYNC(h);
    return AZR_OK;
}

// ---- root noise -----------------------------------------------------------------------------------------
extern "C" int azr_mcts_set_root_noise(azr_engine* h, const float* eta)
{
    ENTER(h);
    if (eta && h->host.gumbel_m > 0) return bad_argument(h, "azr_mcts_set_root_noise: a Gumbel search is in force (azr_mcts_set_gumbel), which takes no root noise");
    const size_t sz = (size_t)h->d.G * MOVES * sizeof(float);
    if (eta) H2D(h, h->d.root_eta, eta, sz);
    else HIPCHK(h, hipMemsetAsync(h->d.root_eta, 0, sz, h->stream));
    SYNC(h);
    h->host.noise = eta != nullptr;
    if (h->mode == 2) h->mode = 0;   // the array was a running self-play's: that self-play is over (azr_selfplay_start* begins the next)
    return AZR_OK;
}

// alpha of a Dirichlet draw: a number in (0, 10]; `off_ok`: or <= 0, which switches the noise off
static int alpha_check(azr_engine* h, const char* who, float alpha, bool off_ok)
{
    if (alpha <= DIR_ALPHA_MAX && (off_ok || alpha > 0.0f)) return AZR_OK;   // (NaN fails)
    return bad_argument(h, std::string(who) + (off_ok ? ": alpha must be a number <= 10 (<= 0 = off)" : ": alpha must be a number in (0, 10]"));
}

extern "C" int azr_selfplay_set_dirichlet(azr_engine* h, float alpha, uint32_t noise_seed)
{
    if (!h) return AZR_E_BAD_HANDLE;
    if (int rc = alpha_check(h, "azr_selfplay_set_dirichlet", alpha, true)) return rc;
    h->sp_set.alpha = alpha > 0.0f ? alpha : 0.0f;
    h->sp_set.noise_seed = noise_seed;
    return AZR_OK;
}

extern "C" int azr_mcts_root_noise(azr_engine* h, float* eta)
{
    ENTER(h);
    if (!eta) return AZR_E_INVALID_ARGUMENT;
    const size_t sz = (size_t)h->d.G * MOVES * sizeof(float);
    if (!options_in_force(h, h->mode).noise) { memset(eta, 0, sz); return AZR_OK; }
    D2H(h, eta, h->d.root_eta, sz);
    SYNC(h);
    return AZR_OK;
}

extern "C" int azr_debug_root_noise(azr_engine* h, float alpha, uint32_t noise_seed, const uint32_t* game_seed, const uint32_t* decision,
                                    const uint64_t* valid, int n, float* eta_out)
{
    ENTER(h);
    if (int rc = alpha_check(h, "azr_debug_root_noise", alpha, false)) return rc;
    if (n < 0 || (n > 0 && (!game_seed || !decision || !valid || !eta_out))) return AZR_E_INVALID_ARGUMENT;
    if (n == 0) return AZR_OK;
    Stage st(h);
    const uint32_t *ds = st.in(game_seed, (size_t)n), *dd = st.in(decision, (size_t)n);
    const uint64_t* dv = st.in(valid, (size_t)n);
    float* eta = st.out(eta_out, (size_t)n * MOVES);
    STAGED_LAUNCH(st, k_debug_root_noise, n, alpha, noise_seed, ds, dd, dv, eta);
    return AZR_OK;
}

// ---- forced playouts and policy target pruning ----------------------------------------------------------
static int forced_k_check(azr_engine* h, const char* who, float k)
{
    if (k != k || k > FORCED_K_MAX) {
        h->err = std::string(who) + ": k must be a number <= 8 (<= 0 = off)";
        return AZR_E_INVALID_ARGUMENT;
    }
    return AZR_OK;
}

extern "C" int azr_mcts_set_forced_playouts(azr_engine* h, float k)
{
    if (!h) return AZR_E_BAD_HANDLE;
    int rc = forced_k_check(h, "azr_mcts_set_forced_playouts", k);
    if (rc) return rc;
    if (k > 0.0f && h->host.gumbel_m > 0) return bad_argument(h, "azr_mcts_set_forced_playouts: a Gumbel search is in force (azr_mcts_set_gumbel), which forces no playouts");
    h->host.forced_k = k > 0.0f ? k : 0.0f;
    return AZR_OK;
}

// a search budget below the settings': n - n % T descents, at least one per search thread and no more than mcts_simulations
static int simulations_check(azr_engine* h, const char* who, const char* what, int n, const char* note)
{
    if (n >= h->cfg.mcts_threads && n <= h->cfg.mcts_simulations) return AZR_OK;
    return bad_argument(h, std::string(who) + ": " + what + " = " + std::to_string(n) + " outside [mcts_threads = " + std::to_string(h->cfg.mcts_threads) +
                               ", mcts_simulations = " + std::to_string(h->cfg.mcts_simulations) + "]" + note);
}

extern "C" int azr_mcts_set_simulations(azr_engine* h, int simulations)
{
    if (!h) return AZR_E_BAD_HANDLE;
    if (int rc = simulations > 0 ? simulations_check(h, "azr_mcts_set_simulations", "simulations", simulations, "") : AZR_OK) return rc;
    h->host.sims = simulations > 0 ? simulations : 0;
    return AZR_OK;
}

extern "C" int azr_selfplay_set_forced_playouts(azr_engine* h, float k, int prune)
{
    if (!h) return AZR_E_BAD_HANDLE;
    int rc = forced_k_check(h, "azr_selfplay_set_forced_playouts", k);
    if (rc) return rc;
    if (prune && !(k > 0.0f)) {
        h->err = "azr_selfplay_set_forced_playouts: prune != 0 needs k > 0 (pruning subtracts forced playouts; there are none)";
        return AZR_E_INVALID_ARGUMENT;
    }
    h->sp_set.forced_k = k > 0.0f ? k : 0.0f;
    h->sp_set.prune = prune != 0;
    return AZR_OK;
}

extern "C" int azr_mcts_pruned_policy(azr_engine* h, float* pi, uint32_t* n_pruned)
{
    ENTER(h);
    if (!pi) return AZR_E_INVALID_ARGUMENT;
    const Dev d = search_view(h, h->mode);
    const size_t sz = (size_t)h->d.G * MOVES;
    Stage st(h);
    uint32_t* dn = st.out(n_pruned, sz);
    float* dp = st.out(pi, sz);
    STAGED_LAUNCH(st, k_pruned_policy, h->d.G, d, dn, dp);
    return AZR_OK;
}

extern "C" int azr_selfplay_start_games_from_states(azr_engine* h, uint32_t base_seed, uint64_t games)
{
    ENTER(h);
    if (games == 0) return AZR_E_INVALID_ARGUMENT;
    return selfplay_start(h, base_seed, games, 1);
}

// ---- policy surprise weighting ----------------------------------------------------------------------------
// share: a number <= 1 (<= 0 = off); when on, max_weight in [1, 64]
static int surprise_check(azr_engine* h, const char* who, float share, float max_weight)
{
    if (share != share || max_weight != max_weight || share > 1.0f)
        return bad_argument(h, std::string(who) + ": share must be a number <= 1 (<= 0 = off) and max_weight a number");
    if (share > 0.0f && !(max_weight >= 1.0f && max_weight <= PSW_MAX_WEIGHT))
        return bad_argument(h, std::string(who) + ": max_weight must lie in [1, 64]");
    return AZR_OK;
}

extern "C" int azr_selfplay_set_surprise_weighting(azr_engine* h, float share, float max_weight, uint32_t seed)
{
    if (!h) return AZR_E_BAD_HANDLE;
    if (int rc = surprise_check(h, "azr_selfplay_set_surprise_weighting", share, max_weight)) return rc;
    const bool on = share > 0.0f;
    h->sp_set.psw_share = on ? share : 0.0f;
    h->sp_set.psw_max = on ? max_weight : 1.0f;
    h->sp_set.psw_seed = seed;
    return AZR_OK;
}

extern "C" int azr_debug_surprise_weights(azr_engine* h, float share, float max_weight, uint32_t seed, const float* pi, const float* prior,
                                          const uint64_t* valid, const uint32_t* game_len, const uint32_t* game_seed, int games,
                                          float* kl_out, float* w_out, uint32_t* copies_out)
{
    ENTER(h);
    if (int rc = surprise_check(h, "azr_debug_surprise_weights", share, max_weight)) return rc;
    if (!(share > 0.0f)) return bad_argument(h, "azr_debug_surprise_weights: share must lie in (0, 1]");
    if (games < 0 || (games > 0 && (!game_len || !game_seed))) return AZR_E_INVALID_ARGUMENT;
    std::vector<uint32_t> first;
    size_t rows;
    if (!first_rows(game_len, games, first, rows)) return bad_argument(h, "azr_debug_surprise_weights: more than 2^31 - 1 records");
    if (rows > 0 && (!pi || !prior || !valid || !kl_out || !w_out || !copies_out)) return AZR_E_INVALID_ARGUMENT;
    if (rows == 0) return AZR_OK;
    Stage st(h);
    const float *dpi = st.in(pi, rows * MOVES), *dprior = st.in(prior, rows * MOVES);
    const uint64_t* dv = st.in(valid, rows);
    const uint32_t *df = st.in(first.data(), (size_t)games), *dl = st.in(game_len, (size_t)games), *ds = st.in(game_seed, (size_t)games);
    float *dk = st.out(kl_out, rows), *dw = st.out(w_out, rows);
    uint32_t* dc = st.out(copies_out, rows);
    STAGED_LAUNCH(st, k_debug_surprise, games, share, max_weight, seed, dpi, dprior, dv, df, dl, ds, dk, dw, dc);
    return AZR_OK;
}

// ---- value mix ------------------------------------------------------------------------------------------
// q_share: a number <= 1 (<= 0 = off)
static int value_mix_check(azr_engine* h, const char* who, float q_share)
{
    if (q_share != q_share || q_share > 1.0f) return bad_argument(h, std::string(who) + ": q_share must be a number <= 1 (<= 0 = off)");
    return AZR_OK;
}

extern "C" int azr_selfplay_set_value_mix(azr_engine* h, float q_share)
{
    if (!h) return AZR_E_BAD_HANDLE;
    if (int rc = value_mix_check(h, "azr_selfplay_set_value_mix", q_share)) return rc;
    h->sp_set.q_share = q_share > 0.0f ? q_share : 0.0f;
    return AZR_OK;
}

extern "C" int azr_debug_value_mix(azr_engine* h, float q_share, const uint32_t* N, const float* Q, const uint64_t* valid, const float* z,
                                   int rows, float* q_out, uint8_t* has_q_out, float* z_out)
{
    ENTER(h);
    if (int rc = value_mix_check(h, "azr_debug_value_mix", q_share)) return rc;
    if (!(q_share > 0.0f)) return bad_argument(h, "azr_debug_value_mix: q_share must lie in (0, 1]");
    if (rows < 0 || (rows > 0 && (!N || !Q || !valid || !z || !q_out || !has_q_out || !z_out))) return AZR_E_INVALID_ARGUMENT;
    if (rows == 0) return AZR_OK;
    const size_t n = (size_t)rows;
    Stage st(h);
    const uint32_t* dn = st.in(N, n * MOVES);
    const float* dq = st.in(Q, n * MOVES);
    const uint64_t* dv = st.in(valid, n);
    const float* dz = st.in(z, n);
    float* oq = st.out(q_out, n);
    uint8_t* oh = st.out(has_q_out, n);
    float* oz = st.out(z_out, n);
    STAGED_LAUNCH(st, k_debug_value_mix, rows, q_share, dn, dq, dv, dz, oq, oh, oz);
    return AZR_OK;
}

// ---- resignation ----------------------------------------------------------------------------------------
// numbers; when on (streak > 0): q_resign in [-1, 1], streak <= 255, holdout_share in [0, 1]
static int resign_check(azr_engine* h, const char* who, float q_resign, int streak, float holdout_share)
{
    if (q_resign != q_resign || holdout_share != holdout_share)
        return bad_argument(h, std::string(who) + ": q_resign and holdout_share must be numbers");
    if (streak <= 0) return AZR_OK;
    if (!(q_resign >= -1.0f && q_resign <= 1.0f)) return bad_argument(h, std::string(who) + ": q_resign must lie in [-1, 1]");
    if (streak > 255) return bad_argument(h, std::string(who) + ": streak must be at most 255 (<= 0 = off)");
    if (!(holdout_share >= 0.0f && holdout_share <= 1.0f)) return bad_argument(h, std::string(who) + ": holdout_share must lie in [0, 1]");
    return AZR_OK;
}

extern "C" int azr_selfplay_set_resign(azr_engine* h, float q_resign, int streak, float holdout_share, uint32_t seed)
{
    if (!h) return AZR_E_BAD_HANDLE;
    if (int rc = resign_check(h, "azr_selfplay_set_resign", q_resign, streak, holdout_share)) return rc;
    const bool on = streak > 0;
    h->sp_set.resign_streak = on ? streak : 0;
    h->sp_set.resign_q = on ? q_resign : 0.0f;
    h->sp_set.resign_holdout = on ? holdout_share : 0.0f;
    h->sp_set.resign_seed = seed;
    return AZR_OK;
}

extern "C" int azr_selfplay_resign_stats(azr_engine* h, azr_resign_stats* out)
{
    ENTER(h);
    if (!out) return AZR_E_INVALID_ARGUMENT;
    std::vector<unsigned long long> rows((size_t)h->d.G * 4);
    D2H(h, rows.data(), h->d.resign_stats, rows.size() * sizeof(unsigned long long));
    SYNC(h);
    memset(out, 0, sizeof *out);
    for (size_t g = 0; g < (size_t)h->d.G; g++) {
        out->resigned += rows[g * 4]; out->holdout_games += rows[g * 4 + 1];
        out->holdout_would_resign += rows[g * 4 + 2]; out->holdout_not_lost += rows[g * 4 + 3];
    }
    return AZR_OK;
}

extern "C" int azr_selfplay_resign_state(azr_engine* h, uint8_t* run_host, uint8_t* first_host, uint8_t* holdout_host)
{
    ENTER(h);
    if (!run_host || !first_host || !holdout_host) return AZR_E_INVALID_ARGUMENT;
    const size_t G = (size_t)h->d.G;
    if (h->mode != 2 || h->d.resign_streak <= 0) {
        memset(run_host, 0, 2 * G); memset(first_host, 255, G); memset(holdout_host, 0, G);
        return AZR_OK;
    }
    Stage st(h);
    uint8_t *dr = st.out(run_host, 2 * G), *df = st.out(first_host, G), *dh = st.out(holdout_host, G);
    STAGED_LAUNCH(st, k_resign_state, h->d.G, h->d, dr, df, dh);
    return AZR_OK;
}

extern "C" int azr_debug_resign(azr_engine* h, float q_resign, int streak, float holdout_share, uint32_t seed, const float* q,
                                const uint8_t* has_q, const uint8_t* player, const uint32_t* game_len, const uint32_t* game_seed, int games,
                                int32_t* resign_row_out, uint8_t* resigner_out, uint8_t* holdout_out)
{
    ENTER(h);
    if (int rc = resign_check(h, "azr_debug_resign", q_resign, streak, holdout_share)) return rc;
    if (streak <= 0) return bad_argument(h, "azr_debug_resign: streak must lie in [1, 255]");
    if (games < 0 || (games > 0 && (!game_len || !game_seed || !resign_row_out || !resigner_out || !holdout_out))) return AZR_E_INVALID_ARGUMENT;
    if (games == 0) return AZR_OK;
    std::vector<uint32_t> first;
    size_t rows;
    if (!first_rows(game_len, games, first, rows)) return bad_argument(h, "azr_debug_resign: more than 2^31 - 1 decisions");
    if (rows > 0 && (!q || !has_q || !player)) return AZR_E_INVALID_ARGUMENT;
    const size_t n = (size_t)games;
    Stage st(h);   // (no decision at all: the three row arrays are empty, and the kernel still runs over the games)
    const float* dq = st.in(q, rows);
    const uint8_t *dh = st.in(has_q, rows), *dp = st.in(player, rows);
    const uint32_t *df = st.in(first.data(), n), *dl = st.in(game_len, n), *ds = st.in(game_seed, n);
    int32_t* orow = st.out(resign_row_out, n);
    uint8_t *owho = st.out(resigner_out, n), *ohold = st.out(holdout_out, n);
    STAGED_LAUNCH(st, k_debug_resign, games, q_resign, (uint32_t)streak, resign_threshold_of(holdout_share), seed, dq, dh, dp, df, dl, ds, orow, owho, ohold);
    return AZR_OK;
}

// ---- Gumbel root search ---------------------------------------------------------------------------------
// numbers; m in [0, 43]; when on (m > 0): c_visit >= 0, c_scale > 0
static int gumbel_check(azr_engine* h, const char* who, int m, float c_visit, float c_scale)
{
    if (!(c_visit - c_visit == 0.0f) || !(c_scale - c_scale == 0.0f)) return bad_argument(h, std::string(who) + ": c_visit and c_scale must be finite numbers");
    if (m < 0 || m > MOVES) return bad_argument(h, std::string(who) + ": m = " + std::to_string(m) + " outside [0, 43] (0 = off)");
    if (m > 0 && !(c_visit >= 0.0f && c_scale > 0.0f)) return bad_argument(h, std::string(who) + ": c_visit must be >= 0 and c_scale > 0");
    return AZR_OK;
}

extern "C" int azr_selfplay_set_gumbel(azr_engine* h, int m, float c_visit, float c_scale, uint32_t seed)
{
    if (!h) return AZR_E_BAD_HANDLE;
    if (int rc = gumbel_check(h, "azr_selfplay_set_gumbel", m, c_visit, c_scale)) return rc;
    h->sp_set.gumbel_m = m;
    h->sp_set.gumbel_cvisit = m > 0 ? c_visit : 0.0f;
    h->sp_set.gumbel_cscale = m > 0 ? c_scale : 0.0f;
    h->sp_set.gumbel_seed = seed;
    return AZR_OK;
}

extern "C" int azr_mcts_set_gumbel(azr_engine* h, int m, float c_visit, float c_scale)
{
    ENTER(h);
    if (int rc = gumbel_check(h, "azr_mcts_set_gumbel", m, c_visit, c_scale)) return rc;
    if (m > 0 && (h->host.noise || h->host.forced_k > 0.0f))
        return bad_argument(h, std::string("azr_mcts_set_gumbel: ") + (h->host.noise ? "a root noise vector (azr_mcts_set_root_noise)" : "forced playouts (azr_mcts_set_forced_playouts)") +
                                   " is in force, which a Gumbel search does not go with");
    const bool toggles = (m > 0) != (h->host.gumbel_m > 0);
    if (m > 0) { if (int rc = gumbel_alloc(h)) return rc; }
    h->host.gumbel_m = m;
    h->host.gumbel_cvisit = m > 0 ? c_visit : 0.0f;
    h->host.gumbel_cscale = m > 0 ? c_scale : 0.0f;
    if (m == 0) h->host.gumbel_tree = false;
    if (toggles) {   // no node without the net's value is searched by a Gumbel search: the trees start empty
        LAUNCH(h, k_tree_clear, h->d);
        if (h->mode == 2) h->mode = 0;   // (a running self-play's trees are gone with them)
    }
    SYNC(h);
    return AZR_OK;
}

// 0 or 1, or the refusal
static int gumbel_tree_check(azr_engine* h, const char* who, int on)
{
    return on == 0 || on == 1 ? AZR_OK : bad_argument(h, std::string(who) + ": on = " + std::to_string(on) + " is not 0 or 1");
}

extern "C" int azr_selfplay_set_gumbel_tree(azr_engine* h, int on)
{
    if (!h) return AZR_E_BAD_HANDLE;
    if (int rc = gumbel_tree_check(h, "azr_selfplay_set_gumbel_tree", on)) return rc;
    h->sp_set.gumbel_tree = on;
    return AZR_OK;
}

extern "C" int azr_mcts_set_gumbel_tree(azr_engine* h, int on)
{
    ENTER(h);
    if (int rc = gumbel_tree_check(h, "azr_mcts_set_gumbel_tree", on)) return rc;
    if (h->host.gumbel_m <= 0) return bad_argument(h, "azr_mcts_set_gumbel_tree: no host-stepped Gumbel search is in force (azr_mcts_set_gumbel with m > 0)");
    h->host.gumbel_tree = on != 0;   // the trees stay: every node a GUMBEL step expanded has its vhat either way
    return AZR_OK;
}

extern "C" int azr_mcts_set_root_gumbel(azr_engine* h, const float* g_host)
{
    ENTER(h);
    if (int rc = gumbel_alloc(h)) return rc;
    const size_t sz = (size_t)h->d.G * MOVES * sizeof(float);
    if (g_host) H2D(h, h->d.root_g, g_host, sz);
    else HIPCHK(h, hipMemsetAsync(h->d.root_g, 0, sz, h->stream));
    SYNC(h);
    if (h->mode == 2) h->mode = 0;   // the array was a running self-play's: that self-play is over
    return AZR_OK;
}

extern "C" int azr_mcts_root_gumbel(azr_engine* h, float* g_host)
{
    ENTER(h);
    if (!g_host) return AZR_E_INVALID_ARGUMENT;
    const size_t sz = (size_t)h->d.G * MOVES * sizeof(float);
    if (!options_in_force(h, h->mode).gumbel || !h->d.root_g) { memset(g_host, 0, sz); return AZR_OK; }
    D2H(h, g_host, h->d.root_g, sz);
    SYNC(h);
    return AZR_OK;
}

// a Gumbel search's settings in force (a running self-play's, else the host-stepped ones), or the reason there are none
static int gumbel_view(azr_engine* h, const char* who, Dev& d)
{
    d = search_view(h, h->mode);
    if (d.gumbel_m <= 0 || !d.root_g || !d.root_n0) {
        h->err = std::string(who) + ": no Gumbel search is in force (azr_mcts_set_gumbel, or a self-play started under azr_selfplay_set_gumbel)";
        return AZR_E_STATE;
    }
    return AZR_OK;
}

extern "C" int azr_mcts_gumbel_policy(azr_engine* h, float* pi_host, float* qhat_host)
{
    ENTER(h);
    if (!pi_host) return AZR_E_INVALID_ARGUMENT;
    Dev d;
    if (int rc = gumbel_view(h, "azr_mcts_gumbel_policy", d)) return rc;
    const size_t sz = (size_t)h->d.G * MOVES;
    Stage st(h);
    float *dq = st.out(qhat_host, sz), *dp = st.out(pi_host, sz);
    STAGED_LAUNCH(st, k_gumbel_policy, h->d.G, d, dq, dp);
    return AZR_OK;
}

extern "C" int azr_mcts_gumbel_pick(azr_engine* h, uint8_t* moves_host)
{
    ENTER(h);
    if (!moves_host) return AZR_E_INVALID_ARGUMENT;
    Dev d;
    if (int rc = gumbel_view(h, "azr_mcts_gumbel_pick", d)) return rc;
    LAUNCH_OUT(h, moves_host, (size_t)h->d.G, uint8_t, k_gumbel_pick, d);
    return AZR_OK;
}

extern "C" int azr_debug_root_gumbel(azr_engine* h, uint32_t seed, const uint32_t* game_seed, const uint32_t* decision, const uint64_t* valid,
                                     const uint8_t* greedy, int rows, float* g_out)
{
    ENTER(h);
    if (rows < 0 || (rows > 0 && (!game_seed || !decision || !valid || !greedy || !g_out))) return AZR_E_INVALID_ARGUMENT;
    if (rows == 0) return AZR_OK;
    const size_t n = (size_t)rows;
    Stage st(h);
    const uint32_t *ds = st.in(game_seed, n), *dd = st.in(decision, n);
    const uint64_t* dv = st.in(valid, n);
    const uint8_t* dg = st.in(greedy, n);
    float* go = st.out(g_out, n * MOVES);
    STAGED_LAUNCH(st, k_debug_root_gumbel, rows, seed, ds, dd, dv, dg, go);
    return AZR_OK;
}

extern "C" int azr_debug_gumbel_select(azr_engine* h, int m, int n, float c_visit, float c_scale, const uint32_t* N, const uint32_t* N0,
                                       const uint32_t* act, const float* Q, const float* P, const float* g, const float* vhat,
                                       const uint64_t* valid, const uint32_t* claim, int rows, uint8_t* move_out, uint32_t* cv_out)
{
    ENTER(h);
    if (int rc = gumbel_check(h, "azr_debug_gumbel_select", m, c_visit, c_scale)) return rc;
    if (m <= 0 || n <= 0) return bad_argument(h, "azr_debug_gumbel_select: m must lie in [1, 43] and n be positive");
    if (rows < 0 || (rows > 0 && (!N || !N0 || !act || !Q || !P || !g || !vhat || !valid || !claim || !move_out || !cv_out))) return AZR_E_INVALID_ARGUMENT;
    if (rows == 0) return AZR_OK;
    const size_t r = (size_t)rows;
    Stage st(h);
    const uint32_t *dN = st.in(N, r * MOVES), *dN0 = st.in(N0, r * MOVES), *dact = st.in(act, r * MOVES);
    const float *dQ = st.in(Q, r * MOVES), *dP = st.in(P, r * MOVES), *dg = st.in(g, r * MOVES), *dvh = st.in(vhat, r);
    const uint64_t* dv = st.in(valid, r);
    const uint32_t* dc = st.in(claim, r);
    uint8_t* om = st.out(move_out, r);
    uint32_t* oc = st.out(cv_out, r);
    STAGED_LAUNCH(st, k_debug_gumbel_select, rows, (uint32_t)m, (uint32_t)n, c_visit, c_scale, dN, dN0, dact, dQ, dP, dg, dvh, dv, dc, om, oc);
    return AZR_OK;
}

extern "C" int azr_debug_gumbel_tree_select(azr_engine* h, float c_visit, float c_scale, const uint32_t* N, const uint32_t* act, const float* Q,
                                            const float* P, const float* vhat, const uint64_t* valid, int rows, uint8_t* move_out, float* score_out)
{
    ENTER(h);
    if (int rc = gumbel_check(h, "azr_debug_gumbel_tree_select", 1, c_visit, c_scale)) return rc;
    if (rows < 0 || (rows > 0 && (!N || !act || !Q || !P || !vhat || !valid || !move_out || !score_out))) return AZR_E_INVALID_ARGUMENT;
    if (rows == 0) return AZR_OK;
    const size_t r = (size_t)rows;
    Stage st(h);
    const uint32_t *dN = st.in(N, r * MOVES), *dact = st.in(act, r * MOVES);
    const float *dQ = st.in(Q, r * MOVES), *dP = st.in(P, r * MOVES), *dvh = st.in(vhat, r);
    const uint64_t* dv = st.in(valid, r);
    uint8_t* om = st.out(move_out, r);
    float* os = st.out(score_out, r * MOVES);
    STAGED_LAUNCH(st, k_debug_gumbel_tree_select, rows, c_visit, c_scale, dN, dact, dQ, dP, dvh, dv, om, os);
    return AZR_OK;
}

extern "C" int azr_debug_exp32(azr_engine* h, const float* x, int n, float* out)
{
    ENTER(h);
    if (n < 0 || (n > 0 && (!x || !out))) return AZR_E_INVALID_ARGUMENT;
    if (n == 0) return AZR_OK;
    Stage st(h);
    const float* dx = st.in(x, (size_t)n);
    float* dout = st.out(out, (size_t)n);
    STAGED_LAUNCH(st, k_debug_exp32, (n + 63) / 64, dx, n, dout);
    return AZR_OK;
}

// ---- playout cap ----------------------------------------------------------------------------------------
extern "C" int azr_selfplay_set_playout_cap(azr_engine* h, float full_prob, int fast_simulations, uint32_t cap_seed)
{
    if (!h) return AZR_E_BAD_HANDLE;
    if (int rc = full_prob_check(h, "azr_selfplay_set_playout_cap", full_prob, " (>= 1 = off)")) return rc;
    const bool on = full_prob < 1.0f && fast_simulations > 0;
    if (int rc = on ? simulations_check(h, "azr_selfplay_set_playout_cap", "fast_simulations", fast_simulations,
                                        " (F - F % T descents would be none, or more than a full decision's)") : AZR_OK) return rc;
    h->sp_set.cap_prob = on ? full_prob : 1.0f;
    h->sp_set.cap_fast_sims = on ? fast_simulations : 0;
    h->sp_set.cap_seed = cap_seed;
    return AZR_OK;
}

extern "C" int azr_selfplay_decision_kind(azr_engine* h, uint8_t* full_host)
{
    ENTER(h);
    if (!full_host) return AZR_E_INVALID_ARGUMENT;
    if (!options_in_force(h, h->mode).cap) { memset(full_host, 1, (size_t)h->d.G); return AZR_OK; }
    LAUNCH_OUT(h, full_host, (size_t)h->d.G, uint8_t, k_decision_kind, h->d);
    return AZR_OK;
}

extern "C" int azr_debug_playout_cap(azr_engine* h, float full_prob, uint32_t cap_seed, const uint32_t* game_seed, const uint32_t* decision,
                                     int n, uint8_t* full_out)
{
    ENTER(h);
    if (int rc = full_prob_check(h, "azr_debug_playout_cap", full_prob, "")) return rc;
    if (n < 0 || (n > 0 && (!game_seed || !decision || !full_out))) return AZR_E_INVALID_ARGUMENT;
    if (n == 0) return AZR_OK;
    Stage st(h);
    const uint32_t *ds = st.in(game_seed, (size_t)n), *dd = st.in(decision, (size_t)n);
    uint8_t* full = st.out(full_out, (size_t)n);
    STAGED_LAUNCH(st, k_debug_playout_cap, (n + 63) / 64, cap_threshold_of(full_prob), cap_seed, ds, dd, n, full);
    return AZR_OK;
}

extern "C" int azr_selfplay_start_from_states(azr_engine* h, uint32_t base_seed)
{
    ENTER(h);
    return selfplay_start(h, base_seed, 0, 1);
}

extern "C" int azr_selfplay_start(azr_engine* h, uint32_t base_seed)
{
    ENTER(h);
    return selfplay_start(h, base_seed, 0);
}

extern "C" int azr_selfplay_start_games(azr_engine* h, uint32_t base_seed, uint64_t games)
{
    ENTER(h);
    if (games == 0) return AZR_E_INVALID_ARGUMENT;
    return selfplay_start(h, base_seed, games);
}

extern "C" int azr_selfplay_run(azr_engine* h, int passes)
{
    ENTER(h);
    if (h->mode != 2) { h->err = "azr_selfplay_run: call azr_selfplay_start first"; return AZR_E_STATE; }
    if (!h->weights_set) { h->err = "azr_selfplay_run: no weights"; return AZR_E_STATE; }
    // launches timed with HIP events, spread evenly over the run.  A sample, not every pass: an event is a marker packet the
    // queue has to retire, and five of them per pass cost ~18 us of a 1.1 ms pass.
    const int nprof = std::min(passes, PROF_MAX);
    for (ProfEvents& e : h->ev)
        for (hipEvent_t* x : {&e.tree0, &e.tree1, &e.net1, &e.tower0, &e.tower1})
            if (!*x) HIPCHK(h, hipEventCreate(x));
    const int stride = passes > nprof ? passes / nprof : 1;
    int k = 0;
    const int GT = h->d.G * h->d.T;
    for (int p = 0; p < passes; p++) {
        // Quota mode (azr_selfplay_start_games): once every game has been started the slots go idle one by one.  From then
        // on a pass evaluates the waiting leaf slots only (listed by the tree step, one count read-back per pass) and the
        // tile plan follows the shrinking batch — a launch over 1024 mostly idle slots costs as much as a full one.
        if (h->d.sp_quota && !h->sp_tail && p % 32 == 0) {
            unsigned long long started = 0;
            D2H(h, &started, h->d.sp_started, sizeof started);
            SYNC(h);
            h->sp_tail = started >= h->d.sp_quota;
            h->d.sp_compact = h->sp_tail ? 1 : 0;
        }
        int n_eval = GT;
        const int* map = nullptr;
        const bool prof = (p % stride == 0) && k < nprof;
        if (h->sp_tail) HIPCHK(h, hipMemsetAsync(h->d.leaf_count, 0, sizeof(int), h->stream));
        const ProfEvents* ev = prof ? &h->ev[k] : nullptr;   // this pass's events, if it is a sampled one
        if (ev) HIPCHK(h, hipEventRecord(ev->tree0, h->stream));
        if (int rc = launch_tree_step(h, h->d, true, h->sp)) return rc;
        if (ev) HIPCHK(h, hipEventRecord(ev->tree1, h->stream));
        if (h->sp_tail) {
            D2H(h, &n_eval, h->d.leaf_count, sizeof(int));
            SYNC(h);
            map = h->d.leaf_list;
            if (n_eval == 0) {   // nothing waits for the net: every game of the quota is over
                if (ev) HIPCHK(h, hipEventRecord(ev->net1, h->stream));
                break;
            }
        }
        h->pe_tower0 = ev ? ev->tower0 : nullptr;
        h->pe_tower1 = ev ? ev->tower1 : nullptr;
        int rc = net_forward_ex(h, h->d.leaf_in, LEAF_STRIDE, n_eval, h->d.net_pi, h->d.net_v, map, h->stream);
        h->pe_tower0 = h->pe_tower1 = nullptr;
        if (rc) return rc;
        if (ev) { HIPCHK(h, hipEventRecord(ev->net1, h->stream)); k++; }
    }
    SYNC(h);
    double tn = 0, tt = 0, tw = 0;
    const bool tower_timed = h->cfg.net_dtype == AZR_NET_BF16 || h->cfg.net_dtype == AZR_NET_F32X || h->cfg.net_dtype == AZR_NET_F16;   // one kernel = one net forward, bracketed by events
    for (int i = 0; i < k; i++) {
        float a = 0, b = 0, c = 0;
        const ProfEvents& ev = h->ev[i];
        HIPCHK(h, hipEventElapsedTime(&a, ev.tree0, ev.tree1));
        HIPCHK(h, hipEventElapsedTime(&b, ev.tree1, ev.net1));
        if (tower_timed) HIPCHK(h, hipEventElapsedTime(&c, ev.tower0, ev.tower1));
        tt += a; tn += b; tw += c;
    }
    h->prof_tower_ms = k ? (float)(tw / k) : 0;
    h->prof_launches = k;
    h->prof_tree_ms = k ? (float)(tt / k) : 0;
    h->prof_net_ms = k ? (float)(tn / k) : 0;
    return AZR_OK;
}

extern "C" int azr_profile_last_run(azr_engine* h, float* net_ms, float* tree_ms, int* launches)
{
    if (!h) return AZR_E_BAD_HANDLE;
    // net_ms: the dominant kernel alone (k_tower_bf16) when the bf16 path is active, else the whole fp32 forward
    if (net_ms) *net_ms = h->prof_tower_ms > 0 ? h->prof_tower_ms : h->prof_net_ms;
    if (tree_ms) *tree_ms = h->prof_tree_ms;
    if (launches) *launches = h->prof_launches;
    return AZR_OK;
}

extern "C" int azr_selfplay_counters(azr_engine* h, azr_counters* out)
{
    ENTER(h);
    if (!out) return AZR_E_INVALID_ARGUMENT;
    std::vector<Counters> rows(h->d.G);
    D2H(h, rows.data(), h->d.counters, rows.size() * sizeof(Counters));
    SYNC(h);
    Counters c;
    memset(&c, 0, sizeof c);
    for (const Counters& r : rows) {
        c.simulations += r.simulations; c.evaluations += r.evaluations; c.levels += r.levels; c.decisions += r.decisions;
        c.games_finished += r.games_finished; c.samples += r.samples; c.nodes_dropped += r.nodes_dropped; c.errors += r.errors;
        c.ring_dropped += r.ring_dropped;
    }
    out->simulations = c.simulations; out->evaluations = c.evaluations; out->levels = c.levels;
    out->decisions = c.decisions; out->games_finished = c.games_finished; out->samples = c.samples;
    out->nodes_dropped = c.nodes_dropped; out->errors = c.errors;
    out->records_dropped = c.ring_dropped;
    out->tower_fallbacks = 0;
    {
        unsigned long long f = 0;
        int rc = net_fallbacks(h, &f);
        if (rc) return rc;
        out->tower_fallbacks = f;
        if (h->opponent) {   // two-net arena: the opponent's launches ran on its own handle
            rc = net_fallbacks(h->opponent, &f);
            if (rc) { h->err = h->opponent->err; return rc; }
            out->tower_fallbacks += f;
        }
    }
    return AZR_OK;
}

// records in the ring (the counter runs past the capacity when flushes were dropped)
static int ring_fill(azr_engine* h, unsigned long long* n)
{
    D2H(h, n, h->d.ring_count, 8);
    SYNC(h);
    if (*n > h->d.ring_cap) *n = h->d.ring_cap;
    return AZR_OK;
}

extern "C" int azr_samples_drain(azr_engine* h, void* rec265, size_t cap, size_t* n_out)
{
    ENTER(h);
    unsigned long long n = 0;
    int rc = ring_fill(h, &n);
    if (rc) return rc;
    if (!rec265) cap = (size_t)n;   // no buffer: discard everything (reset of the ring)
    size_t take = std::min((size_t)n, cap);
    if (take && rec265) D2H(h, rec265, h->d.ring, take * AZR_RECORD_BYTES);
    const unsigned long long left = n - take;
    if (left) {  // partial drain: the records that did not fit move to the front of the ring and stay
        DevBuf tmp;
        HIPCHK(h, tmp.alloc((size_t)left * AZR_RECORD_BYTES));
        HIPCHK(h, hipMemcpyAsync(tmp.p, h->d.ring + take * AZR_RECORD_BYTES, (size_t)left * AZR_RECORD_BYTES, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->d.ring, tmp.p, (size_t)left * AZR_RECORD_BYTES, hipMemcpyDeviceToDevice, h->stream));
        SYNC(h);
    }
    HIPCHK(h, hipMemcpyAsync(h->d.ring_count, &left, 8, hipMemcpyHostToDevice, h->stream));
    if (h->arena_rec) {   // the drained records give their ring room back (no kernel runs: the stream is synchronised)
        unsigned long long claim = 0;
        D2H(h, &claim, h->d.ring_count + 1, 8);
        SYNC(h);
        claim = claim > take ? claim - take : 0;
        HIPCHK(h, hipMemcpyAsync(h->d.ring_count + 1, &claim, 8, hipMemcpyHostToDevice, h->stream));
    }
    SYNC(h);
    if (n_out) *n_out = take;
    return AZR_OK;
}

extern "C" int azr_samples_device_view(azr_engine* h, void** dev_ptr, size_t* n_out)
{
    ENTER(h);
    unsigned long long n = 0;
    int rc = ring_fill(h, &n);
    if (rc) return rc;
    if (dev_ptr) *dev_ptr = h->d.ring;
    if (n_out) *n_out = (size_t)n;
    return AZR_OK;
}

extern "C" int azr_samples_copy_device(azr_engine* h, void* dst_device, size_t cap, size_t* n_out)
{
    ENTER(h);
    unsigned long long n = 0;
    int rc = ring_fill(h, &n);
    if (rc) return rc;
    const size_t take = std::min((size_t)n, cap);
    if (take && !dst_device) return AZR_E_INVALID_ARGUMENT;
    if (take) HIPCHK(h, hipMemcpyAsync(dst_device, h->d.ring, take * AZR_RECORD_BYTES, hipMemcpyDeviceToDevice, h->stream));
    SYNC(h);
    if (n_out) *n_out = take;
    return AZR_OK;
}

extern "C" int azr_device_synchronize(azr_engine* h)
{
    ENTER(h);
    SYNC(h);
    return AZR_OK;
}

// ---- arena: GameGroup::playGames (game/game.cpp:256-312) ----------------------------------------------------------
extern "C" int azr_arena_start(azr_engine* h, int player1, int player2, int games, int games_per_slot_cap, int mirror_games,
                               uint32_t base_seed)
{
    ENTER(h);
    if (player1 < 0 || player1 > 3 || player2 < 0 || player2 > 3 || games < 0) return AZR_E_INVALID_ARGUMENT;
    if (mirror_games < AZR_MIRROR_OFF || mirror_games > AZR_MIRROR_CONCURRENT) { h->err = "azr_arena_start: mirror_games must be AZR_MIRROR_OFF / _SEQUENTIAL / _CONCURRENT"; return AZR_E_INVALID_ARGUMENT; }
    if (mirror_games == AZR_MIRROR_CONCURRENT && h->d.G < 2) { h->err = "azr_arena_start: AZR_MIRROR_CONCURRENT needs at least 2 slots (a pair's halves play on slots 2j and 2j + 1)"; return AZR_E_INVALID_ARGUMENT; }
    if (player1 == player2 && (player1 == AZR_PLAYER_ALPHAZERO || player1 == AZR_PLAYER_ALPHAZERO_B)) {
        h->err = "azr_arena_start: two AlphaZero players need one tree each: use AZR_PLAYER_ALPHAZERO vs AZR_PLAYER_ALPHAZERO_B "
                 "(azr_arena_set_opponent_net(h, h) for the same network on both sides)";
        return AZR_E_STATE;
    }
    const bool usesA = player1 == AZR_PLAYER_ALPHAZERO || player2 == AZR_PLAYER_ALPHAZERO;
    const bool usesB = player1 == AZR_PLAYER_ALPHAZERO_B || player2 == AZR_PLAYER_ALPHAZERO_B;
    if (usesA && !h->weights_set) { h->err = "azr_arena_start: no weights"; return AZR_E_STATE; }
    if (usesB && (!h->opponent || !h->opponent->weights_set)) {
        h->err = "azr_arena_start: AZR_PLAYER_ALPHAZERO_B needs azr_arena_set_opponent_net with a handle that has weights";
        return AZR_E_STATE;
    }
    // a Gumbel side of this arena (a setting for a player that does not play leaves the arena what it is)
    const bool gumbel = (usesA && h->arena_gumbel_set.side[0].m > 0) || (usesB && h->arena_gumbel_set.side[1].m > 0);
    if (gumbel && h->arena_script)
        return bad_argument(h, "azr_arena_start: a Gumbel search (azr_arena_set_gumbel) does not go with scripted-sample collection "
                               "(azr_arena_collect_scripted_samples): switch one of them off");
    if (gumbel) { if (int rc = gumbel_alloc_n0(h)) return rc; }   // (g = 0: no root_g)
    Dev& d = h->d;
    // both sides' Gumbel settings and player B's search settings as they stand now: a running arena never sees a later change
    h->arena_gumbel = gumbel;
    h->arena_gumbel_run = h->arena_gumbel_set;
    d.search2_simulations = h->opp_simulations >= 0 ? h->opp_simulations : d.search.simulations;
    d.search2_hp = h->opp_hp >= 0 ? h->opp_hp : d.search.hp;
    d.nodes2 = usesB ? h->tree2[0] ? (uint8_t*)h->tree2[0] : nullptr : nullptr;
    h->arena_rec = h->arena_script;
    if (d.arena_collect || h->arena_rec) HIPCHK(h, hipMemsetAsync(d.ring_count, 0, 2 * sizeof(unsigned long long), h->stream));
    d.kind0 = player1; d.kind1 = player2; d.arena_total = games; d.arena_slot_cap = games_per_slot_cap;
    d.arena_mirror = mirror_games; d.base_seed = base_seed;
    h->mode = 3;
    HIPCHK(h, hipMemsetAsync(d.arena_taken, 0, sizeof(int), h->stream));
    HIPCHK(h, hipMemsetAsync(d.leaf_count, 0, 4 * sizeof(int), h->stream));
    h->arena_pass = 0;
    HIPCHK(h, hipMemsetAsync(d.arena_res, 0, 8 * sizeof(int), h->stream));
    HIPCHK(h, hipMemsetAsync(d.counters, 0, (size_t)d.G * sizeof(Counters), h->stream));
    HIPCHK(h, hipMemsetAsync(d.resign_stats, 0, (size_t)d.G * 4 * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(d.alog_status, 0, (size_t)d.G * ALOG, h->stream));
    LAUNCH(h, k_arena_start, d);
    SYNC(h);
    h->arena_open = true;
    return AZR_OK;
}

// slots that have played out their share of the arena (arena_state 2)
static int arena_idle_slots(azr_engine* h, int* idle)
{
    std::vector<uint32_t> st(h->d.G);
    HIPCHK(h, ctl_field_get(h, offsetof(Ctl, arena_state), st.data()));
    SYNC(h);
    *idle = (int)std::count(st.begin(), st.end(), 2u);
    return AZR_OK;
}

extern "C" int azr_arena_run(azr_engine* h, int passes, int* finished_out)
{
    ENTER(h);
    if (h->mode != 3) { h->err = "azr_arena_run: call azr_arena_start first"; return AZR_E_STATE; }
    const int GT = h->d.G * h->d.T;
    const bool needs_net = h->d.kind0 == AZR_PLAYER_ALPHAZERO || h->d.kind1 == AZR_PLAYER_ALPHAZERO;
    const bool any_net = needs_net || h->d.nodes2;   // (neither: scripted players only, a pass is the step alone)
    // Up to 256 waiting leaves on the 16-bit towers and the NET_F32X tower, in any pairing of them: the net launches read the tree step's
    // leaf counts from device memory themselves (net_forward_counted), so a pass is queued without a read-back and the host looks at the
    // slots' states once per CHUNK passes — the passes of a slot that went idle meanwhile end at their first instruction.  An arena with a
    // NET_F32 side reads back.  (Test build, AZR_ARENA_COUNTED=0: the read-back form; =2: AZR_E_STATE where the read-back form would run.)
    // (At most min(slots, games) slots ever play: an engine of 512 slots that plays 100 compare games has at most 200 leaves waiting.)
    const int NB_MAX = std::min(h->d.G, std::max(1, h->d.arena_total)) * h->d.T;
    const int form = hook_env_int("AZR_ARENA_COUNTED", 1);
    const bool can_count = net_forward_counted_ok(h, NB_MAX) && (!h->d.nodes2 || net_forward_counted_ok(h->opponent, NB_MAX));
    const bool counted = form != 0 && can_count && any_net;
    if (form == 2 && !can_count && any_net) { h->err = "azr_arena_run: AZR_ARENA_COUNTED=2 and this arena reads back"; return AZR_E_STATE; }
    constexpr int CHUNK = 16;
    if (h->d.nodes2 && !h->arena_ev) HIPCHK(h, hipEventCreateWithFlags(&h->arena_ev, hipEventDisableTiming));
    if (h->d.nodes2 && counted && !h->arena_ev2) HIPCHK(h, hipEventCreateWithFlags(&h->arena_ev2, hipEventDisableTiming));
    int idle = 0;
    for (int p = 0; p < passes; p++) {
        bool look;   // at the slots' states after this pass: the arena may be over
        if (counted) {
            // the counts of this pass go to row (pass & 1) of leaf_count — zero since the pass before the last (or azr_arena_start) — and the
            // step zeroes the other row for the next pass: no memset between a pass's launches either
            const int row = 2 * (int)(h->arena_pass++ & 1u);
            Dev e = h->d;
            e.lc_base = row; e.lc_zero = 2 - row;
            ARENA_STEP(h, e);
            const int* cnt_dev = h->d.leaf_count + row;
            const bool beside = h->d.nodes2 && h->opponent != h;   // two launches on two streams (one handle on both sides: one stream, one after the other)
            // what each launch has to know of the one beside it: its count word and the charge per board pair of its batch, from that
            // handle's plan (test build, AZR_ARENA_BESIDE_WGPP=N: N instead — 1 = the workgroups k_tower_fx<2> really spends on a pair,
            // 256 = the whole chip; tests and measurements of the side-by-side rule)
            const int wgpp_hook = hook_env_int("AZR_ARENA_BESIDE_WGPP", 0);
            const int wgpp_opp = !beside ? 0 : wgpp_hook > 0 ? wgpp_hook : net_counted_wgs_per_pair(h->opponent);
            const int wgpp_own = !beside ? 0 : wgpp_hook > 0 ? wgpp_hook : net_counted_wgs_per_pair(h);
            if (h->d.nodes2) {   // the opponent's net on the opponent's stream, side by side with this one's: after the tree step, before the next
                HIPCHK(h, hipEventRecord(h->arena_ev2, h->stream));
                HIPCHK(h, hipStreamWaitEvent(h->opponent->stream, h->arena_ev2, 0));
                int rc = net_forward_counted(h->opponent, h->d.leaf_in, LEAF_STRIDE, NB_MAX, cnt_dev + 1, beside ? cnt_dev : nullptr, wgpp_own, h->d.net_pi, h->d.net_v, h->d.leaf_list + GT, h->opponent->stream);
                if (rc) { h->err = h->opponent->err; return rc; }
                HIPCHK(h, hipEventRecord(h->arena_ev, h->opponent->stream));
            }
            int rc = net_forward_counted(h, h->d.leaf_in, LEAF_STRIDE, NB_MAX, cnt_dev, beside ? cnt_dev + 1 : nullptr, wgpp_opp, h->d.net_pi, h->d.net_v, h->d.leaf_list, h->stream);
            if (rc) return rc;
            if (h->d.nodes2) HIPCHK(h, hipStreamWaitEvent(h->stream, h->arena_ev, 0));
            look = p % CHUNK == CHUNK - 1 && p + 1 < passes;
        } else {   // one count read-back per pass: every net evaluates the waiting leaf slots of its own player only
            int cnt[2] = {0, 0};
            const size_t words = !any_net ? 0 : h->d.nodes2 ? sizeof cnt : sizeof cnt[0];   // the count words in play: one per net
            if (words) HIPCHK(h, hipMemsetAsync(h->d.leaf_count, 0, words, h->stream));
            ARENA_STEP(h, h->d);
            if (words) {
                D2H(h, cnt, h->d.leaf_count, words);
                SYNC(h);
            }
            // The two launches are independent (own weights, disjoint leaf slots) and small — an arena of 100 games is
            // 1 board per workgroup on fewer than half of the CUs each — so they run side by side: this net on this
            // handle's stream, the opponent's on the opponent's; the next tree step waits for both.  (The tree step that
            // wrote the leaves has completed: the count read-back above synchronised the stream.)
            int rc = net_forward_ex(h, h->d.leaf_in, LEAF_STRIDE, cnt[0], h->d.net_pi, h->d.net_v, h->d.leaf_list, h->stream);   // (no launch for a count of 0)
            if (rc) return rc;
            if (cnt[1] > 0) {
                rc = net_forward_ex(h->opponent, h->d.leaf_in, LEAF_STRIDE, cnt[1], h->d.net_pi, h->d.net_v, h->d.leaf_list + GT, h->opponent->stream);
                if (rc) { h->err = h->opponent->err; return rc; }
                HIPCHK(h, hipEventRecord(h->arena_ev, h->opponent->stream));
                HIPCHK(h, hipStreamWaitEvent(h->stream, h->arena_ev, 0));
            }
            // nobody waits for a net: either every slot is idle (quota exhausted), or only scripted players moved or waited for ring room
            look = any_net && cnt[0] == 0 && cnt[1] == 0;
        }
        if (look) {
            int rc = arena_idle_slots(h, &idle);
            if (rc) return rc;
            if (idle == h->d.G) break;
        }
    }
    int rc = arena_idle_slots(h, &idle);
    if (rc) return rc;
    if (idle == h->d.G) h->arena_open = false;
    if (finished_out) *finished_out = idle == h->d.G;
    return AZR_OK;
}

extern "C" int azr_arena_set_opponent_net(azr_engine* h, azr_engine* other)
{
    ENTER(h);
    if (!other) {
        h->opponent = nullptr;
        h->opp_simulations = -1;   // azr_arena_set_opponent_search's setting goes with the opponent (read by the next azr_arena_start)
        h->opp_hp = -1.0f;
        h->arena_gumbel_set.side[1] = GumbelSide{};   // ... and so does azr_arena_set_gumbel's for player B
        return AZR_OK;
    }
    // Depth and element type are the opponent's own business: its launches run with its own weights, context and activation buffers on
    // this handle's leaves (96-byte NNInputData in, fp32 pi / v out — the same for every tower).  Its buffers must hold this handle's batch.
    if (other->cfg.device != h->cfg.device || other->d.G * other->d.T < h->d.G * h->d.T) {
        h->err = "azr_arena_set_opponent_net: the opponent handle must be on the same device and have >= leaf slots";
        return AZR_E_INVALID_ARGUMENT;
    }
    Dev& d = h->d;
    if (!h->tree2[0]) {  // the second AlphaZeroPlayer's tree per slot + the per-net leaf lists
        const size_t G = d.G, C = d.C;
        uint8_t* n2 = nullptr; uint32_t *t2 = nullptr, *h2 = nullptr, *tb2 = nullptr, *tc2 = nullptr; uint16_t* f2 = nullptr;
        HIPCHK(h, dmalloc(&n2, G * C * NODE_BYTES)); h->tree2[0] = n2;
        HIPCHK(h, dmalloc(&t2, G * C)); h->tree2[1] = t2;
        HIPCHK(h, dmalloc(&h2, G * C)); h->tree2[2] = h2;
        HIPCHK(h, dmalloc(&tb2, G * d.H)); h->tree2[3] = tb2;
        HIPCHK(h, dmalloc(&f2, G * C)); h->tree2[4] = f2;
        HIPCHK(h, dmalloc(&tc2, G * 4)); h->tree2[5] = tc2;
        HIPCHK(h, hipMemsetAsync(t2, 0, G * C * sizeof(uint32_t), h->stream));
        HIPCHK(h, hipMemsetAsync(tb2, 0, G * d.H * sizeof(uint32_t), h->stream));
        HIPCHK(h, hipMemsetAsync(tc2, 0, G * 4 * sizeof(uint32_t), h->stream));
        d.touch2 = t2; d.nhash2 = h2; d.table2 = tb2; d.freel2 = f2; d.tctl2 = tc2;
        SYNC(h);
    }
    h->opponent = other;
    return AZR_OK;
}

extern "C" int azr_arena_set_opponent_search(azr_engine* h, int mcts_simulations, float hp_exploration)
{
    ENTER(h);
    if (h->mode == 3 && h->arena_open) {
        h->err = "azr_arena_set_opponent_search: an arena is running (set it before azr_arena_start or after the arena has finished)";
        return AZR_E_STATE;
    }
    if (hp_exploration != hp_exploration) { h->err = "azr_arena_set_opponent_search: hp_exploration is not a number"; return AZR_E_INVALID_ARGUMENT; }
    const int T = h->d.T;
    int sims = -1;
    if (mcts_simulations >= 0) {
        if (mcts_simulations < T) {   // count = S - S % T would be 0, as at azr_engine_create
            h->err = "azr_arena_set_opponent_search: mcts_simulations = " + std::to_string(mcts_simulations) + " < mcts_threads = " +
                     std::to_string(T) + " (S - S % T simulations would be none)";
            return AZR_E_INVALID_ARGUMENT;
        }
        // player B's tree lives in this handle's second node pool, sized like the first: a budget the pool was not made for would
        // drop expansions.  Refused, not clamped.
        const long long want_nodes = 16ll * ((long long)mcts_simulations + 1);
        if (want_nodes > (long long)h->d.C) {
            h->err = "azr_arena_set_opponent_search: mcts_simulations = " + std::to_string(mcts_simulations) + " needs a node pool of 16 * (" +
                     std::to_string(mcts_simulations) + " + 1) = " + std::to_string(want_nodes) + " nodes per game, this handle's holds " +
                     std::to_string(h->d.C) + ": create the handle with a larger node_capacity";
            return AZR_E_INVALID_ARGUMENT;
        }
        sims = mcts_simulations - mcts_simulations % T;   // alphazero_mcts.cpp:265, per player
    }
    h->opp_simulations = sims;   // azr_arena_start hands them to the kernels
    h->opp_hp = hp_exploration < 0 ? -1.0f : hp_exploration;
    return AZR_OK;
}

extern "C" int azr_arena_set_gumbel(azr_engine* h, int player, int m, float c_visit, float c_scale, int tree)
{
    ENTER(h);
    if (h->mode == 3 && h->arena_open) {
        h->err = "azr_arena_set_gumbel: an arena is running (set it before azr_arena_start or after the arena has finished)";
        return AZR_E_STATE;
    }
    if (player != AZR_PLAYER_ALPHAZERO && player != AZR_PLAYER_ALPHAZERO_B)
        return bad_argument(h, "azr_arena_set_gumbel: player = " + std::to_string(player) + " is neither AZR_PLAYER_ALPHAZERO nor AZR_PLAYER_ALPHAZERO_B");
    if (int rc = gumbel_check(h, "azr_arena_set_gumbel", m, c_visit, c_scale)) return rc;
    if (tree != 0 && tree != 1) return bad_argument(h, "azr_arena_set_gumbel: tree = " + std::to_string(tree) + " is not 0 or 1");
    if (tree && m == 0)
        return bad_argument(h, "azr_arena_set_gumbel: the Gumbel selection below the root (tree = 1) needs the Gumbel root search (m > 0)");
    GumbelSide& a = h->arena_gumbel_set.side[player == AZR_PLAYER_ALPHAZERO_B ? 1 : 0];   // azr_arena_start hands them to the kernels
    a.m = m;
    a.c_visit = m > 0 ? c_visit : 0.0f;
    a.c_scale = m > 0 ? c_scale : 0.0f;
    a.tree = tree;
    return AZR_OK;
}

extern "C" int azr_arena_collect_samples(azr_engine* h, int on)
{
    if (!h) return AZR_E_BAD_HANDLE;
    h->d.arena_collect = on ? 1 : 0;
    return AZR_OK;
}

extern "C" int azr_arena_collect_scripted_samples(azr_engine* h, int on)
{
    if (!h) return AZR_E_BAD_HANDLE;
    h->arena_script = on != 0;
    return AZR_OK;
}

extern "C" int azr_arena_results(azr_engine* h, azr_game_results* out)
{
    ENTER(h);
    if (!out) return AZR_E_INVALID_ARGUMENT;
    int r[8];
    D2H(h, r, h->d.arena_res, sizeof r);
    SYNC(h);
    out->count = r[0]; out->draw = r[1]; out->win[0] = r[2]; out->win_and_started[0] = r[3];
    out->win[1] = r[4]; out->win_and_started[1] = r[5];
    return AZR_OK;
}

extern "C" int azr_arena_log(azr_engine* h, int32_t* games_per_slot, int8_t* status, uint16_t* rounds, void* finals160)
{
    ENTER(h);
    const int G = h->d.G;
    if (games_per_slot) HIPCHK(h, ctl_field_get(h, offsetof(Ctl, slot_games), games_per_slot));
    if (status) D2H(h, status, h->d.alog_status, (size_t)G * ALOG);
    if (rounds) D2H(h, rounds, h->d.alog_rounds, (size_t)G * ALOG * 2);
    if (finals160) {
        DevBuf b;
        HIPCHK(h, b.alloc((size_t)G * ALOG * 160));
        hipLaunchKernelGGL(k_export160, dim3(G * ALOG), dim3(64), 0, h->stream, h->d, (const uint8_t*)h->d.alog_final, (uint8_t*)b.p);
        HIPCHK(h, hipGetLastError());
        D2H(h, finals160, b.p, (size_t)G * ALOG * 160);
        SYNC(h);
    }
    SYNC(h);
    return AZR_OK;
}
