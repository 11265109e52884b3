// azr_search.hpp — device code of the per-game search step: tree views, the Ctl line in registers, per-game counters, consuming the
// net's answers, descents, one search round, record staging and the self-play game turnover.  Included by azr_engine.hip only.
#pragma once
#include "azr_internal.hpp"
#include "azr_cap.hpp"
#include "azr_noise.hpp"
#include "azr_surprise.hpp"
#include "azr_resign.hpp"
#include "azr_gumbel.hpp"

namespace azr {

__device__ __forceinline__ Tree tree_of(const Dev& E, int g)
{
    Tree t;
    t.C = E.C; t.H = E.H; t.DMAX = E.DMAX;
#ifdef AZR_TEST_HOOKS
    t.hash_and = E.hash_and; t.hash_or = E.hash_or;
#endif
    t.nodes = E.nodes + (size_t)g * E.C * NODE_BYTES;
    t.touch = E.touch + (size_t)g * E.C;
    t.nhash = E.nhash + (size_t)g * E.C;
    t.table = E.table + (size_t)g * E.H;
    t.freel = E.freel + (size_t)g * E.C;
    t.path = E.path + (size_t)g * E.T * E.DMAX;  // thread 0's stack; thread_tree() selects thread k's
    return t;
}

// the opponent AlphaZero player's tree of game g (two-net arena)
__device__ __forceinline__ Tree tree2_of(const Dev& E, int g)
{
    Tree t = tree_of(E, g);
    t.nodes = E.nodes2 + (size_t)g * E.C * NODE_BYTES;
    t.touch = E.touch2 + (size_t)g * E.C;
    t.nhash = E.nhash2 + (size_t)g * E.C;
    t.table = E.table2 + (size_t)g * E.H;
    t.freel = E.freel2 + (size_t)g * E.C;
    return t;
}
// tree 2's allocator / trim state lives outside the (full) Ctl line; it is swapped into the Ctl fields the tree
// functions use while that tree is being worked on
struct TreeCtl { uint32_t search_id, nfree, hiwater; };
__device__ __forceinline__ void swap_tree_ctl(Ctl& c, TreeCtl& x)
{
    uint32_t a = c.search_id, b = c.nfree, d = c.hiwater;
    c.search_id = x.search_id; c.nfree = x.nfree; c.hiwater = x.hiwater;
    x.search_id = a; x.nfree = b; x.hiwater = d;
}

__device__ __forceinline__ void ctl_load(Ctl& c, const Ctl* src)
{
    const uint32_t* p = reinterpret_cast<const uint32_t*>(src);
    uint32_t w = p[lane_id() & 31u];
    c.mode = rdl(w, 0); c.search_id = rdl(w, 1); c.sims_done = rdl(w, 2); c.pending = rdl(w, 3);
    c.sims_started = rdl(w, 4); c.nfree = rdl(w, 5); c.hiwater = rdl(w, 6); c.search_done = rdl(w, 7);
    c.rng = rdl(w, 8); c.game_no = rdl(w, 9); c.nsamples = rdl(w, 10); c.status = (int32_t)rdl(w, 11);
    c.error = rdl(w, 12); c.last_move = rdl(w, 13); c.decisions = rdl(w, 14); c.seed = rdl(w, 15);
    c.arena_state = rdl(w, 16); c.player_start = rdl(w, 17); c.pair_phase = rdl(w, 18); c.turn_started = rdl(w, 19);
    c.search_active = rdl(w, 20); c.slot_games = rdl(w, 21); c.dup_dropped = rdl(w, 22);
#pragma unroll
    for (int k = 0; k < MAX_THREADS; k++) c.plen[k] = rdl(w, 23 + k);
    c.search_tree = rdl(w, 31);
}
// c.plen[k] with a wave-uniform runtime k, without indexing the register array
__device__ __forceinline__ uint32_t plen_get(const Ctl& c, int k)
{
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < MAX_THREADS; i++) v = k == i ? c.plen[i] : v;
    return v;
}
__device__ __forceinline__ void plen_set(Ctl& c, int k, uint32_t v)
{
#pragma unroll
    for (int i = 0; i < MAX_THREADS; i++) c.plen[i] = k == i ? v : c.plen[i];
}
__device__ __forceinline__ Tree thread_tree(const Tree& t, int k)
{
    Tree tk = t;
    tk.path = t.path + (size_t)k * t.DMAX;
    return tk;
}
__device__ __forceinline__ void ctl_store(const Ctl& c, Ctl* dst)
{
    uint32_t l = lane_id();
    uint32_t w = 0;
    w = l == 0 ? c.mode : w; w = l == 1 ? c.search_id : w; w = l == 2 ? c.sims_done : w; w = l == 3 ? c.pending : w;
    w = l == 4 ? c.sims_started : w; w = l == 5 ? c.nfree : w; w = l == 6 ? c.hiwater : w; w = l == 7 ? c.search_done : w;
    w = l == 8 ? c.rng : w; w = l == 9 ? c.game_no : w; w = l == 10 ? c.nsamples : w; w = l == 11 ? (uint32_t)c.status : w;
    w = l == 12 ? c.error : w; w = l == 13 ? c.last_move : w; w = l == 14 ? c.decisions : w; w = l == 15 ? c.seed : w;
    w = l == 16 ? c.arena_state : w; w = l == 17 ? c.player_start : w; w = l == 18 ? c.pair_phase : w;
    w = l == 19 ? c.turn_started : w; w = l == 20 ? c.search_active : w; w = l == 21 ? c.slot_games : w;
    w = l == 22 ? c.dup_dropped : w;
#pragma unroll
    for (int k = 0; k < MAX_THREADS; k++) w = l == 23u + k ? c.plen[k] : w;
    w = l == 31 ? c.search_tree : w;
    if (l < 32) reinterpret_cast<uint32_t*>(dst)[l] = w;
}

// packs one finished game's staged records into the 265-byte on-disk layout (record_byte); QMIX: their z blended with the staged
// root values (azr_valuemix.hpp)
template <bool QMIX = false>
__device__ __forceinline__ void flush_samples(const Dev& E, int g, uint32_t n, int status, unsigned long long& dropped)
{
    if (n == 0) return;
    unsigned long long start = 0;
    if (lane_id() == 0) start = atomicAdd(E.ring_count, (unsigned long long)n);
    start = rfl64(start);
    const uint8_t* st = E.stage + (size_t)g * E.SCAP * STAGE_BYTES;
    for (uint32_t r = 0; r < n; r++) {
        unsigned long long slot = start + r;
        if (slot >= E.ring_cap) { dropped += 1; continue; }
        const uint8_t* src = st + (size_t)r * STAGE_BYTES;
        uint8_t* dst = E.ring + (size_t)slot * AZR_RECORD_BYTES;
        uint32_t player = rfl((uint32_t)src[260]);
        const uint32_t zb = record_z_bits<QMIX>(E, g, r, player, status);
        for (uint32_t j = lane_id(); j < AZR_RECORD_BYTES; j += 64) dst[j] = record_byte(src, player, zb, j);
    }
}

struct StepCount {
    unsigned long long sims = 0, evals = 0, levels = 0, dec = 0, games = 0, samples = 0, drop = 0, err = 0, ringdrop = 0;
};

// Counters are kept PER GAME (one 72-byte row each, written by the game's own wave: no atomics) and summed by the host
// when somebody asks (azr_selfplay_counters).  One shared row bumped with atomics made every pass end with G x 4..9
// same-address device atomics, which the L2 retires one by one (~12 ns each): 20 us of a 47-us tree step at 512 games.
// `count_active`: host-stepped search only (azr_mcts_leaves reads the number of games that wait for the net).
// The row is read-modify-write, and the read is issued when the wave STARTS (counters_begin): at the end of a step the wave's stores
// are still draining, and a load issued behind them waits for every one of them (memory operations of a wave retire in order) —
// 3.7 us of an average mid-game wave, 9 us of the slow ones the launch waits for (profiles/r03_tree_step_profile.txt).
__device__ __forceinline__ unsigned long long counters_begin(const Dev& E, int g)
{
    const uint32_t l = lane_id();
    return l < 9 ? reinterpret_cast<const unsigned long long*>(E.counters + g)[l] : 0ull;
}
__device__ __forceinline__ void flush_counters(const Dev& E, int g, const Ctl& c, const StepCount& k, bool count_active, unsigned long long base)
{
    if (count_active && lane_id() == 0 && c.pending) atomicAdd(E.active, 1u);
    const uint32_t l = lane_id();
    unsigned long long d = 0;
    d = l == 0 ? k.sims : d; d = l == 1 ? k.evals : d; d = l == 2 ? k.levels : d; d = l == 3 ? k.dec : d; d = l == 4 ? k.games : d;
    d = l == 5 ? k.samples : d; d = l == 6 ? k.drop : d; d = l == 7 ? k.err : d; d = l == 8 ? k.ringdrop : d;
    if (l < 9 && d) {
        unsigned long long* row = reinterpret_cast<unsigned long long*>(E.counters + g);
        row[l] = base + d;
    }
}

// One training record of the decision taken at `root`, in the staged layout flush_samples packs when the game ends (encode88(root) |
// pi[43] | player to move), into the slot's staging buffer; a record past the buffer's end is counted, not staged.
__device__ __forceinline__ void stage_sample(const Dev& E, int g, Ctl& c, const WS& root, float pi, StepCount& k)
{
    if (c.nsamples < (uint32_t)E.SCAP) {
        uint8_t* rec = E.stage + ((size_t)g * E.SCAP + c.nsamples) * STAGE_BYTES;
        encode88(root, rec);
        const uint32_t l = lane_id();
        if (l < MOVES) reinterpret_cast<float*>(rec + 88)[l] = pi;
        if (l == 0) rec[260] = (uint8_t)root.cur;
        c.nsamples++;
    } else k.ringdrop++;
}

// Policy surprise weighting: the surprise of the record stage_sample stages next, into the float beside its staging slot (nothing for
// a record past the buffer's end, which stage_sample counts and drops).  pi: what goes into the record; P: the root's stored prior row.
__device__ __forceinline__ void stage_surprise(const Dev& E, int g, const Ctl& c, float pi, float P, uint64_t valid)
{
    if (c.nsamples >= (uint32_t)E.SCAP) return;
    const float kl = record_surprise(pi, P, valid);
    if (lane_id() == 0) E.stage_kl[(size_t)g * E.SCAP + c.nsamples] = kl;
}

// Value mix: the root value of the record stage_sample stages next, into the float beside its staging slot, NaN for a root without a
// completed visit (nothing for a record past the buffer's end).  N, Q: the root node's rows as the search left them, N the unpruned count.
__device__ __forceinline__ void stage_root_value(const Dev& E, int g, const Ctl& c, uint32_t N, float Q, uint64_t valid)
{
    if (c.nsamples >= (uint32_t)E.SCAP) return;
    bool has_q;
    const float q = root_value(N, Q, valid, has_q);
    if (lane_id() == 0) E.stage_q[(size_t)g * E.SCAP + c.nsamples] = has_q ? q : __uint_as_float(0x7FC00000u);
}

// Resignation at a recorded decision of player p of slot g's game, after its record has been staged: the rule of include/azr.h on the
// root value of the finished search (N the unpruned count) and the slot's state `rs`, which goes back to memory.  True: the game ends
// here, p gives it up.  A held-out game only remembers who would have been first.
__device__ __forceinline__ bool resign_decision(const Dev& E, int g, const Ctl& c, uint32_t& rs, uint32_t p, uint32_t N, float Q, uint64_t valid)
{
    bool has_q;
    const float q = root_value(N, Q, valid, has_q);
    bool resigned = false;
    if (resign_update(rs, p, q, has_q, E.resign_q, (uint32_t)E.resign_streak)) {
        if (resign_holdout(E.resign_threshold, E.resign_seed, c.seed)) resign_note_first(rs, p);
        else resigned = true;
    }
    if (lane_id() == 0) E.resign_state[g] = rs;
    return resigned;
}

// Lists this slot's waiting leaves (leaf slot g * T + thread, in thread order) behind those of the slots that came first: one atomic per
// slot on `count_word`, then a popcount scatter into `list`.  The net of the pass evaluates the listed slots only.
__device__ __forceinline__ void list_pending(const Dev& E, int g, const Ctl& c, int* count_word, int* list)
{
    if (!c.pending) return;
    int base = 0;
    if (lane_id() == 0) base = atomicAdd(count_word, (int)__builtin_popcount(c.pending));
    base = (int)rfl((uint32_t)base);
    const uint32_t l = lane_id();
    if (l < (uint32_t)E.T && ((c.pending >> l) & 1u)) list[base + (int)__builtin_popcount(c.pending & ((1u << l) - 1u))] = g * E.T + (int)l;
}

// AlphaZeroMCTS::search leaf branch, after the future resolved (alphazero_mcts.cpp:350-356): expand + backup, for every
// search thread with a pending leaf, in thread order.  A state another thread has added meanwhile is dropped
// (StateSimulationsStorage::add, alphazero_mcts.cpp:203-215) and its value still backed up.
// GUMBEL: the net's value of the expanded node — for its mover, what tree_backup takes — is kept in the node (azr_gumbel.hpp).
template <bool GUMBEL = false>
__device__ __forceinline__ void consume_pending(const Dev& E, int g, const Tree& t, Ctl& c, StepCount& k)
{
    if (!c.pending) return;
    const uint32_t l = lane_id();
    for (int th = 0; th < E.T; th++) {
        if (!((c.pending >> th) & 1u)) continue;
        const size_t slot = (size_t)g * E.T + th;
        float pi = E.net_pi[slot * PI_STRIDE + (l < MOVES ? l : 0)];
        float v = rdlf(E.net_v[slot], 0);
        uint64_t valid = rfl64(E.leaf_valid[slot]);
        uint32_t kd = reinterpret_cast<const uint32_t*>(E.leaf_key + slot * GREC)[l & 15u];
        uint32_t h = rfl(E.leaf_hash[slot]);
        TP(1);
        if (E.T > 1 && tree_lookup(t, kd, h) != NO_NODE) c.dup_dropped++;
        else {
            TP(2);
            float prior = normalize_prior(pi, valid);
            TP(3);
            // The ROOT finds the pool full (every pooled node survived the trim and the new root is none of them).  Dropping it would have
            // the next pass ask for it again, for ever: the search could not start.  The tree is emptied for it, as by clearNodes, and
            // the evicted nodes are counted.  No path is in flight: the threads start after the root.
            if (plen_get(c, th) == 0 && c.nfree == 0 && (int)c.hiwater >= t.C) {
                k.drop += c.hiwater;
                tree_clear(t, c);
            }
            if (GUMBEL) {
                const uint32_t idx = tree_expand(t, c, kd, h, valid, prior);
                if (idx == NO_NODE) k.drop++;
                else node_set_vhat(t, idx, v);
            } else if (tree_expand(t, c, kd, h, valid, prior) == NO_NODE) k.drop++;
        }
        TP(4);
        k.evals++;
        const uint32_t plen = plen_get(c, th);
        if (plen > 0) {  // plen == 0: this was setRootState's root expansion (not a simulation)
            tree_backup(thread_tree(t, th), plen, v, false);
            c.sims_done++;
            k.sims++;
        }
        TP(5);
    }
    c.pending = 0;
}

enum : int { RD_DONE = 0, RD_LEAF = 1, RD_FAIL = 2 };

// AlphaZeroMCTS::threadSimulateJob + search (alphazero_mcts.cpp:310-377) for search thread `th`, iteratively: claim the
// next simulation from the counter and descend from the root, repeated until the counter is exhausted (RD_DONE), a leaf
// needs the net (RD_LEAF: leaf record written to slot g * T + th, pending bit set) or a rule error (RD_FAIL).
// `S`: the settings of the tree that is searching (the arena's player B may carry its own budget and PUCT constant).
// NOISE: the game's root noise vector `eta` (lane i <-> move i) enters the first selection of every descent (tree_select).
// FORCED: that selection forces playouts with the factor `fk` (0 = not in this search: a fast decision under a playout cap).
// GUMBEL: that selection is gumbel_select_root's (azr_gumbel.hpp) for the claim index sims_started - 1; `eta` carries the root's g.
// GTREE (with GUMBEL): every later selection of the descent is gumbel_select_tree's, under the root's c_visit and c_scale.
// SIDE (the arena's Gumbel step; without the four above): one descent loop serves both players.  Which of the three selections runs is
// the searching side's setting `sd` (wave-uniform; the steps without SIDE pass none): m > 0 is GUMBEL's, with g = 0 where `eta` goes, and
// tree GTREE's; a side with m = 0 selects by tree_select under `S`, as in a step without any of this.
template <bool NOISE, bool FORCED = false, bool GUMBEL = false, bool GTREE = false, bool SIDE = false>
__device__ __forceinline__ int run_descents(const Dev& E, const Search& S, int g, const Tree& t0, int th, Ctl& c, const WS& root, int8_t* scratch,
                                            StepCount& k, uint32_t& err_out, float eta, float fk = 0.0f, const GumbelSide* sd = nullptr)
{
    const Rules R = E.rules;
    const Tree t = thread_tree(t0, th);
    const size_t slot = (size_t)g * E.T + th;
    static_assert(!SIDE || (!NOISE && !FORCED && !GUMBEL && !GTREE), "SIDE takes the search from the arena's per-side settings alone");
    const GumbelSide side = SIDE ? *sd : GumbelSide{};
    while ((int)c.sims_started < S.simulations) {
        c.sims_started++;  // Counter::hasNext
        WS s = root;
        s.rng = c.rng;
        s.err = 0;
        uint32_t plen = 0;
        bool leaf = false, fail = false;
        TP(6);
        for (;;) {
            int gs = game_status(s, R);
            TP(7);
            if (gs != ST_NOT_ENDED) {
                float v = gs == ST_DRAW ? 0.0f : (gs == (int)s.cur ? 1.0f : -1.0f);
                tree_backup(t, plen, v);
                c.sims_done++;
                k.sims++;
                TP(5);
                break;
            }
            uint64_t valid = valid_moves(s, R);
            TP(8);
            if (valid == 0) { fail = true; s.err = E_INVALID_ARGUMENT; break; }
            uint32_t kd = ws_record_dword(s);
            uint32_t h = key_hash(t, kd);
            TP(9);
            NodeRegs nr;
            uint32_t idx = tree_lookup_node(t, kd, h, nr);
            TP(10);
            if (idx == NO_NODE) {  // leaf: hand the position to the NN service
                encode88(s, E.leaf_in + slot * LEAF_STRIDE);
                const uint32_t l = lane_id();
                if (l < 16) reinterpret_cast<uint32_t*>(E.leaf_key + slot * GREC)[l] = kd;
                if (l == 0) { E.leaf_valid[slot] = valid; E.leaf_hash[slot] = h; }
                leaf = true;
                TP(11);
                break;
            }
            k.levels++;
            uint32_t mv;
            if (SIDE && side.m > 0 && plen == 0)
                mv = gumbel_select_root(t, idx, nr, c.search_id, E.root_n0 + (size_t)g * MOVES, c.sims_started - 1u, (uint32_t)side.m, (uint32_t)S.simulations,
                                        side.c_visit, side.c_scale, eta);
            else if (SIDE && side.tree)
                mv = gumbel_select_tree(nr.W, nr.Q, nr.P, node_vhat(t, idx), (uint64_t)rfl(nr.valid_lo) | ((uint64_t)rfl(nr.valid_hi) << 32),
                                        side.c_visit, side.c_scale, reinterpret_cast<uint32_t*>(node_ptr(t, idx) + ND_N), t.touch + idx, c.search_id);
            else if (GUMBEL && plen == 0)
                mv = gumbel_select_root(t, idx, nr, c.search_id, E.root_n0 + (size_t)g * MOVES, c.sims_started - 1u, (uint32_t)E.gumbel_m,
                                        (uint32_t)S.simulations, E.gumbel_cvisit, E.gumbel_cscale, eta);
            else if (GTREE)
                mv = gumbel_select_tree(nr.W, nr.Q, nr.P, node_vhat(t, idx), (uint64_t)rfl(nr.valid_lo) | ((uint64_t)rfl(nr.valid_hi) << 32),
                                        E.gumbel_cvisit, E.gumbel_cscale, reinterpret_cast<uint32_t*>(node_ptr(t, idx) + ND_N), t.touch + idx, c.search_id);
            else mv = tree_select<NOISE, FORCED>(t, idx, nr, S, c.search_id, scratch, plen == 0, E.noise_eps, eta, fk);
            TP(12);
            if (mv == NONE) { fail = true; s.err = E_LOGIC; break; }
            uint32_t before = s.cur;
#ifdef AZR_TREE_PROF
            const uint32_t ph0 = s.phase;
#endif
            make_move(s, mv, R);
#ifdef AZR_TREE_PROF
            TP(ph0 == PH_FORTIFY ? 22 : ph0 == PH_ATTACK ? 23 : 13);
#endif
            if (s.err) { fail = true; break; }
            if ((int)plen >= t.DMAX) { fail = true; s.err = AZR_E_CAPACITY; break; }
            if (lane_id() == 0) t.path[plen] = idx | (mv << 16) | ((s.cur != before ? 1u : 0u) << 24);
            plen++;
        }
        c.rng = s.rng;
        if (fail) { err_out = s.err; return RD_FAIL; }
        if (leaf) {
            if (plen == 0) c.sims_started--;  // setRootState's root expansion is not one of the S simulations
            c.pending |= 1u << th;
            plen_set(c, th, plen);
            return RD_LEAF;
        }
    }
    return RD_DONE;
}

// One round of AlphaZeroMCTS::simulate for all T search threads of the game, in thread order: every thread without a
// pending leaf runs descents until it blocks on the net.  RD_LEAF = at least one leaf is waiting; RD_DONE = the counter
// is exhausted and every claimed simulation is backed up.
template <bool NOISE, bool FORCED = false, bool GUMBEL = false, bool GTREE = false, bool SIDE = false>
__device__ __forceinline__ int search_round(const Dev& E, const Search& S, int g, const Tree& t, Ctl& c, const WS& root, int8_t* scratch,
                                            StepCount& k, uint32_t& err_out, float eta, float fk = 0.0f, const GumbelSide* sd = nullptr)
{
    for (int th = 0; th < E.T; th++) {
        if ((c.pending >> th) & 1u) continue;
        int r = run_descents<NOISE, FORCED, GUMBEL, GTREE, SIDE>(E, S, g, t, th, c, root, scratch, k, err_out, eta, fk, sd);
        if (r == RD_FAIL) { c.pending = 0; return RD_FAIL; }
        if (r == RD_LEAF && plen_get(c, th) == 0) break;  // root expansion: the threads start after setRootState
    }
    return c.pending ? RD_LEAF : RD_DONE;
}

// N[lane] and the legal mask of the node of `root` (NO_NODE if the root is not in the tree); Q[lane] and P[lane] for who asks (azr_mcts_root_stats)
__device__ __forceinline__ uint32_t root_node(const Tree& t, const WS& root, uint32_t& N, uint64_t& valid, float* Q = nullptr, float* P = nullptr)
{
    uint32_t rkd = ws_record_dword(root);
    uint32_t ridx = tree_lookup(t, rkd, key_hash(t, rkd));
    N = 0; valid = 0;
    if (ridx != NO_NODE) {
        const uint8_t* n = node_ptr(t, ridx);
        const uint32_t l = lane_id();
        N = reinterpret_cast<const uint32_t*>(n + ND_N)[l < MOVES ? l : 0] & N_MASK;
        valid = (uint64_t)rfl(*reinterpret_cast<const uint32_t*>(n + ND_VALID_LO)) |
                ((uint64_t)rfl(*reinterpret_cast<const uint32_t*>(n + ND_VALID_HI)) << 32);
        if (Q) *Q = reinterpret_cast<const float*>(n + ND_Q)[l < MOVES ? l : 0];
        if (P) *P = reinterpret_cast<const float*>(n + ND_P)[l < MOVES ? l : 0];
    }
    return ridx;
}

// the slot's next self-play game.  Unlimited mode: seeds base + g, base + G + g, ...  Quota mode (azr_selfplay_start_games,
// Counter::hasNext of alphazero_trainer.cpp:83): the next game index is a ticket from one atomic counter — exactly
// sp_quota games are started, seeds base .. base + sp_quota - 1, each game a function of its seed alone; a slot that
// draws no ticket goes idle (mode 0).  Under resignation the slot's runs and `first` start over with the game (azr_resign.hpp).
__device__ __forceinline__ void selfplay_next_game(const Dev& E, int g, const Tree& t, Ctl& c, WS& root)
{
    if (E.resign_streak > 0 && lane_id() == 0) E.resign_state[g] = 0u;
    c.game_no++;
    c.seed = E.base_seed + c.game_no * (uint32_t)E.G + (uint32_t)g;
    if (E.sp_quota) {
        unsigned long long ticket = 0;
        if (lane_id() == 0) ticket = atomicAdd(E.sp_started, 1ull);
        ticket = rfl64(ticket);
        if (ticket >= E.sp_quota) { c.mode = 0; c.pending = 0; c.nsamples = 0; return; }
        c.seed = E.base_seed + (uint32_t)ticket;
    }
    ws_blank(root);
    root.rng = rng_seed(c.seed);
    new_game(root);
    c.rng = root.rng;
    c.nsamples = 0; c.decisions = 0; c.sims_done = 0; c.sims_started = 0; c.pending = 0;
    tree_clear(t, c);
}

// the vector of game g's NEW root in a self-play whose steps carry NOISE: stored for azr_mcts_root_noise and handed to the descents; zeros
// for a slot that went idle.  A root that draws gets Dirichlet(E.noise_alpha) for (seed, decision) of the running game over its legal
// moves; one that does not gets the constant vector (DIR_NOISE_VALUE in all 43 entries: the first selection then computes
// eps * DIR_NOISE_VALUE, the constant form's c2, bit for bit).  Every root draws; under a playout cap (CAP) the full ones; with forced
// playouts (FORCED, whose NOISE also serves a self-play without azr_selfplay_set_dirichlet) the full ones of a self-play that set an alpha.
template <bool CAP, bool FORCED>
__device__ __forceinline__ float new_root_noise(const Dev& E, int g, const Ctl& c, const WS& root, bool full)
{
    const bool draw = FORCED ? (full && E.noise_alpha > 0.0f) : CAP ? full : true;
    float eta = 0.0f;
    if (c.mode != 0) eta = draw ? dirichlet_draw(E.noise_alpha, E.noise_seed, c.seed, c.decisions, valid_moves(root, E.rules)) : E.noise_value;
    if (lane_id() < MOVES) E.root_eta[(size_t)g * MOVES + lane_id()] = eta;
    return eta;
}

// g of game g's NEW root in a self-play whose steps carry GUMBEL (azr_gumbel.hpp): stored for azr_mcts_root_gumbel and handed to the
// descents and the decision; zeros for a slot that went idle and for a greedy root (its round above temperature_threshold)
__device__ __forceinline__ float new_root_gumbel(const Dev& E, int g, const Ctl& c, const WS& root)
{
    float gum = 0.0f;
    if (c.mode != 0) gum = gumbel_draw(E.gumbel_seed, c.seed, c.decisions, valid_moves(root, E.rules), (int)root.round > E.search.temperature_threshold);
    if (lane_id() < MOVES) E.root_g[(size_t)g * MOVES + lane_id()] = gum;
    return gum;
}

// N' of the root node `ridx` under policy target pruning (azr_forced.hpp), lane = move: the node's Q, P and sumN word, the root-level
// noised prior of tree_select under the vector `eta`
__device__ __forceinline__ uint32_t root_pruned_counts(const Dev& E, const Search& S, const Tree& t, uint32_t ridx, uint32_t N, uint64_t valid, float eta, float fk)
{
    const uint8_t* n = node_ptr(t, ridx);
    const uint32_t l = lane_id(), ll = l < MOVES ? l : 0;
    const float P = reinterpret_cast<const float*>(n + ND_P)[ll];
    const float Q = reinterpret_cast<const float*>(n + ND_Q)[ll];
    const uint32_t sumN = rfl(*reinterpret_cast<const uint32_t*>(n + ND_SUMN));
    const float noiseP = __fadd_rn(__fmul_rn(S.c1, P), __fmul_rn(E.noise_eps, eta));
    return prune_counts(N, Q, noiseP, valid, sumN, fk, S.hp);
}

}  // namespace azr
