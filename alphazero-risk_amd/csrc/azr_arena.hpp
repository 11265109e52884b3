// azr_arena.hpp — device code of the arena step (k_arena_step / k_arena_step_rec / k_arena_step_gumbel).  Included by azr_engine.hip only.
#pragma once
#include "azr_search.hpp"
// (after azr_internal.hpp: StageRec uses its STAGE_BYTES)
#include "azr_players.hpp"

namespace azr {

// ================================================================================================
// arena: GameGroup::playGames on the device (game/game.cpp:101-312).  One slot = one player pair = one "thread" of
// the reference: games in mirrored pairs with alternating starts, AlphaZeroPlayer::takeTurn (alphazero_player.cpp:3-21)
// through the search of azr_search.hpp, ScriptPlayer / RandomPlayer as wave-resident code (azr_players.hpp).
// ================================================================================================
// ring room for scripted collection (azr_arena_collect_scripted_samples): ring_count[1] = records flushed and not yet drained +
// SCAP per game in progress.  A game is dealt only once its SCAP records are claimed, so a flush always lands inside the ring.
__device__ __forceinline__ bool ring_reserve(const Dev& E)
{
    uint32_t ok = 0;
    if (lane_id() == 0) {
        unsigned long long* claim = E.ring_count + 1;
        unsigned long long cur = atomicAdd(claim, 0ULL);
        while (cur + (unsigned long long)E.SCAP <= E.ring_cap) {
            const unsigned long long prev = atomicCAS(claim, cur, cur + (unsigned long long)E.SCAP);
            if (prev == cur) { ok = 1; break; }
            cur = prev;
        }
    }
    return rfl(ok) != 0;
}
__device__ __forceinline__ void ring_release(const Dev& E, uint32_t n)
{
    if (lane_id() == 0 && n) atomicAdd(E.ring_count + 1, (unsigned long long)(-(long long)n));
}

// a slot's ScriptPlayer state with its five live fields wave-uniform
__device__ __forceinline__ void script_load(ScriptW& p, const ScriptW& src)
{
    p = src;
    p.order = rfl(p.order); p.attacking_set = rfl(p.attacking_set); p.land_to = rfl(p.land_to);
    p.land_from = rfl(p.land_from); p.attack_from_army = rfl(p.attack_from_army);
}

// the shared end of a deal: both AlphaZero players' trees empty, nothing of the game searched or staged yet
__device__ __forceinline__ void arena_begin_game(const Tree& t, const Tree& t2, bool two, Ctl& c, TreeCtl& x2)
{
    tree_clear(t, c);  // AlphaZeroPlayer::newGame
    if (two) { swap_tree_ctl(c, x2); tree_clear(t2, c); swap_tree_ctl(c, x2); }
    c.nsamples = 0;
    c.sims_done = 0; c.sims_started = 0; c.search_active = 0; c.turn_started = 0; c.pending = 0;
    c.arena_state = 1;
}

// SREC: ScriptPlayer / RandomPlayer record their moves (StageRec); without it they get NoRec and this is the arena as it was
// GUMBEL (without SREC): an AlphaZero side of this arena searches by the Gumbel root search with sequential halving
// (azr_arena_set_gumbel, azr_gumbel.hpp; both sides' settings in `A`) under g = 0 — evaluation games draw nothing.  The side that searches is wave-uniform (w): its
// descents take the SIDE round of azr_search.hpp, one loop for both sides, and its decision gumbel_move / gumbel_policy or, with m = 0,
// root_policy / pick_highest as in a step without this.  Every expansion keeps the net's value in the node, in both trees, so that no
// node without one is ever searched (arena_begin_game empties both at every deal).  N0 lives in the slot's root_n0 row: a slot runs
// one search at a time, and claim 0 of every search rewrites it.
template <bool SREC, bool GUMBEL = false>
__device__ __forceinline__ void arena_step(const Dev& E, int8_t* scratch, const ArenaGumbel* A = nullptr)
{
    const int g = blockIdx.x;
    if (E.lc_zero >= 0 && g == 0 && threadIdx.x < 2) E.leaf_count[E.lc_zero + threadIdx.x] = 0;   // the next pass's counts (the last readers are done)
    Ctl c;
    ctl_load(c, &E.ctl[g]);
    if (c.mode != 3 || c.arena_state == 2) return;
    const unsigned long long cnt0 = counters_begin(E, g);
    Tree t = tree_of(E, g);
    const Rules R = E.rules;
    WS root;
    ws_load(root, E.state + (size_t)g * GREC);
    root.rng = c.rng;
    const ScriptW* script = reinterpret_cast<const ScriptW*>(E.script) + (size_t)g * 2;
    ScriptW sp[2];
    script_load(sp[0], script[0]);
    script_load(sp[1], script[1]);
    StepCount k;
    // two-net arena: the opponent AlphaZero player's own tree and its allocator state
    const bool two = E.nodes2 != nullptr;
    const Tree t2 = two ? tree2_of(E, g) : t;
    TreeCtl x2 = {0, 0, 0};
    if (two) {
        const uint32_t w = E.tctl2[(size_t)g * 4 + (lane_id() & 3u)];
        x2.search_id = rdl(w, 0); x2.nfree = rdl(w, 1); x2.hiwater = rdl(w, 2);
    }
    static_assert(!(SREC && GUMBEL), "scripted collection and a Gumbel side do not go together (azr_arena_start refuses the pair)");
    if (c.search_tree) { swap_tree_ctl(c, x2); consume_pending<GUMBEL>(E, g, t2, c, k); swap_tree_ctl(c, x2); }
    else consume_pending<GUMBEL>(E, g, t, c, k);
    for (;;) {
        if (c.arena_state == 0 && E.arena_mirror == AZR_MIRROR_CONCURRENT) {
            // Both games of a mirrored pair at the same time: slot 2j plays half 0 of slot pair j's k-th pair, slot 2j + 1 the
            // mirrored half (include/azr.h).  Nothing in Game orders the two games (game.cpp:238-254); what they share is the
            // deal (game.cpp:170-191), and the deal is a function of the pair's seed, so each half deals for itself.
            const int L = E.G >> 1, lane = g >> 1;
            const uint32_t half = (uint32_t)g & 1u;
            const long long pr = (long long)lane + (long long)c.slot_games * L;   // pairs are assigned statically
            const bool capped = E.arena_slot_cap > 0 && (int)c.slot_games >= E.arena_slot_cap;
            if (capped || g >= 2 * L || pr >= (long long)(E.arena_total / 2)) { c.arena_state = 2; break; }
            if (SREC && !ring_reserve(E)) break;   // no ring room for this game: wait for the next drain, the pair stays this slot's
            const uint32_t pseed = E.base_seed + (uint32_t)pr;
            root.rng = rng_seed(pseed);
            new_game(root);
            if (half) {   // Game::newGame's mirrored branch: invertPlayers of the pair's deal, player 1 starts, own dice stream
                invert_players(root);
                root.rng = rng_seed(pseed + (1u << 30));
            }
            root.cur = half;
            c.player_start = half;
            c.seed = pseed;
            arena_begin_game(t, t2, two, c, x2);
        }
        if (c.arena_state == 0) {  // Game::newGame (game.cpp:170-191) for the next Game::playGames(1)
            if (SREC) {   // ring room first: a slot that has to wait takes nothing from the quota
                const bool capped = c.pair_phase == 0 && E.arena_slot_cap > 0 && (int)c.slot_games >= E.arena_slot_cap;
                if (!capped && !ring_reserve(E)) break;
            }
            if (c.pair_phase == 0) {  // Counter::hasNext(2) (game.cpp:14-26)
                int taken = 0;
                const bool capped = E.arena_slot_cap > 0 && (int)c.slot_games >= E.arena_slot_cap;
                if (!capped && lane_id() == 0) taken = atomicAdd(E.arena_taken, 2);
                taken = (int)rfl((uint32_t)taken);
                if (capped || taken + 2 > E.arena_total) {
                    if (SREC && !capped) ring_release(E, (uint32_t)E.SCAP);
                    c.arena_state = 2;
                    break;
                }
            }
            if (E.arena_mirror && c.player_start != 0) {
                uint32_t keep = root.rng;
                ws_load(root, E.prev_start + (size_t)g * GREC);
                root.rng = keep;
                invert_players(root);
                root.cur = c.player_start;
            } else {
                new_game(root);
                root.cur = c.player_start;
                ws_store(root, E.prev_start + (size_t)g * GREC);
            }
            arena_begin_game(t, t2, two, c, x2);
        }
        // ---- Game::playTurn (game.cpp:112-133)
        int gs = game_status(root, R);
        if (gs != ST_NOT_ENDED) {  // GameResults::addGame (game.cpp:193-213)
            if (lane_id() == 0) {
                atomicAdd(&E.arena_res[0], 1);
                if (gs == ST_DRAW) atomicAdd(&E.arena_res[1], 1);
                if (gs == 0 || gs == 1) {
                    atomicAdd(&E.arena_res[2 + 2 * gs], 1);
                    if ((int)c.player_start == gs) atomicAdd(&E.arena_res[3 + 2 * gs], 1);
                }
                if (c.slot_games < (uint32_t)ALOG) {
                    E.alog_status[(size_t)g * ALOG + c.slot_games] = (int8_t)gs;
                    E.alog_rounds[(size_t)g * ALOG + c.slot_games] = (uint16_t)root.round;
                }
            }
            if (c.slot_games < (uint32_t)ALOG) ws_store(root, E.alog_final + ((size_t)g * ALOG + c.slot_games) * GREC);
            if (SREC) ring_release(E, (uint32_t)E.SCAP - c.nsamples);   // the game's n records stay claimed until they are drained
            if ((SREC || E.arena_collect) && c.nsamples) {  // Player::gameFinished -> NNTrainDataStorage::updateValues for both players
                wave_mem_sync();
                flush_samples(E, g, c.nsamples, gs, k.ringdrop);
                k.samples += c.nsamples;
                c.nsamples = 0;
            }
            c.slot_games++;
            k.games++;
            c.player_start ^= 1u;  // Game::incPlayerStart (the concurrent form sets it per game)
            c.pair_phase ^= 1u;
            c.arena_state = 0;
            continue;
        }
        const uint32_t p = root.cur;
        const int kind = p == 0 ? E.kind0 : E.kind1;
        bool fail = false;
        if (kind == 1) {
            if (SREC) {
                const StageRec rec{E.stage + (size_t)g * E.SCAP * STAGE_BYTES, (uint32_t)E.SCAP, c.nsamples, k.ringdrop};
                if (p == 0) script_take_turn(sp[0], root, R, rec); else script_take_turn(sp[1], root, R, rec);
            } else {
                if (p == 0) script_take_turn(sp[0], root, R, NoRec{}); else script_take_turn(sp[1], root, R, NoRec{});
            }
            fail = root.err != 0 || (root.cur == p && game_status(root, R) == ST_NOT_ENDED);  // "Turn was not incremented"
        } else if (kind == 2) {
            if (SREC) random_take_turn(root, R, StageRec{E.stage + (size_t)g * E.SCAP * STAGE_BYTES, (uint32_t)E.SCAP, c.nsamples, k.ringdrop});
            else random_take_turn(root, R, NoRec{});
            fail = root.err != 0 || (root.cur == p && game_status(root, R) == ST_NOT_ENDED);
        } else {
            const uint32_t w = kind == 3 ? 1u : 0u;   // which AlphaZeroPlayer: its tree and its network
            const Tree& tt = w ? t2 : t;
            if (w) swap_tree_ctl(c, x2);
            // the player's own trimNodes at the start of a turn, setRootState's at the start of every search: at a turn's first decision
            // both run back to back, which leaves an empty tree (tree_trim_twice)
            if (!c.turn_started && !c.search_active) tree_trim_twice(tt, c);
            else if (!c.turn_started || !c.search_active) tree_trim(tt, c);
            c.turn_started = 1;
            if (!c.search_active) { c.sims_done = 0; c.sims_started = 0; c.search_active = 1; }
            c.search_tree = w;
            c.rng = root.rng;
            uint32_t err = 0;
            // every AlphaZeroPlayer owns an AlphaZeroMCTS with its own Settings: player B's simulation count and PUCT constant
            // (azr_arena_set_opponent_search); the noise term is shared, and it is the constant one: evaluation games are played
            // without root noise, whatever azr_mcts_set_root_noise / azr_selfplay_set_dirichlet say
            Search Sw = E.search;
            if (w) { Sw.simulations = E.search2_simulations; Sw.hp = E.search2_hp; }
            const GumbelSide side = GUMBEL ? (w ? A->side[1] : A->side[0]) : GumbelSide{};
            int r = GUMBEL ? search_round<false, false, false, false, true>(E, Sw, g, tt, c, root, scratch, k, err, 0.0f, 0.0f, &side)
                           : search_round<false>(E, Sw, g, tt, c, root, scratch, k, err, 0.0f);
            root.rng = c.rng;
            if (r == RD_LEAF) { if (w) swap_tree_ctl(c, x2); break; }
            if (r == RD_FAIL) { fail = true; root.err = err; }
            else {
                uint32_t N; uint64_t valid;
                uint32_t mv = NONE;
                float Q = 0.0f, P = 0.0f;   // GUMBEL: the root's mean values and stored prior row
                const uint32_t ridx = root_node(tt, root, N, valid, GUMBEL ? &Q : nullptr, GUMBEL ? &P : nullptr);
                if (ridx != NO_NODE) {
                    float pi;
                    if (GUMBEL && side.m > 0) {   // one score serves the move and the record, as in a self-play GUMBEL step
                        const GumbelScore sc = gumbel_score(N, Q, P, node_vhat(tt, ridx), valid, side.c_visit, side.c_scale);
                        mv = gumbel_move(sc, N, E.root_n0[(size_t)g * MOVES + (lane_id() < MOVES ? lane_id() : 0)], 0.0f, valid);
                        pi = gumbel_policy(sc, valid);
                    } else {
                        pi = root_policy(N, valid);
                        mv = pick_highest(pi);
                    }
                    if (E.arena_collect) stage_sample(E, g, c, root, pi, k);  // AlphaZeroPlayer::takeTurn with trainStorage set (alphazero_player.cpp:15-18)
                }
                if (mv != NONE) make_move(root, mv, R); else root.err = E_LOGIC;
                c.search_active = 0;
                c.last_move = mv;
                k.dec++;
                fail = root.err != 0;
                if (root.cur != p || game_status(root, R) != ST_NOT_ENDED) c.turn_started = 0;
            }
            if (w) swap_tree_ctl(c, x2);
        }
        if (fail) {  // the reference would have thrown out of GameGroup: drop the game, start a fresh pair
            k.err++;
            c.error = root.err ? root.err : (uint32_t)E_LOGIC;
            root.err = 0;
            c.player_start = 0; c.pair_phase = 0; c.arena_state = 0;
            c.pending = 0; c.search_active = 0; c.turn_started = 0;
            if (E.arena_mirror == AZR_MIRROR_CONCURRENT) c.slot_games++;   // statically assigned: go on with the slot's next pair
            if (SREC) { ring_release(E, (uint32_t)E.SCAP); c.nsamples = 0; }   // the game's staged records go with it
        }
    }
    if (two && lane_id() == 0) { uint32_t* d2 = E.tctl2 + (size_t)g * 4; d2[0] = x2.search_id; d2[1] = x2.nfree; d2[2] = x2.hiwater; }
    // hand every waiting leaf to the network of the player that is searching (list 0 when there is one network): a pass
    // evaluates the listed slots only — most slots of an arena idle (scripted players' turns, finished quotas)
    const uint32_t tree = two ? c.search_tree : 0u;
    list_pending(E, g, c, &E.leaf_count[E.lc_base + tree], E.leaf_list + (size_t)tree * E.G * E.T);
    c.rng = root.rng;
    ws_store(root, E.state + (size_t)g * GREC);
    {
        ScriptW* dst = reinterpret_cast<ScriptW*>(E.script) + (size_t)g * 2;
        if (lane_id() == 0) { dst[0] = sp[0]; dst[1] = sp[1]; }
    }
    ctl_store(c, &E.ctl[g]);
    flush_counters(E, g, c, k, false, cnt0);
}

}  // namespace azr
