// azr_internal.hpp — engine object shared by the C-ABI translation units (host side).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../include/azr.h"
#include "azr_tree.hpp"

// a failed HIP call ends the C-ABI function that made it: its text goes into the handle's error string, AZR_E_HIP comes back
#define HIPCHK(h, call)                                                                         \
    do {                                                                                        \
        hipError_t e__ = (call);                                                                \
        if (e__ != hipSuccess) {                                                                \
            (void)hipGetLastError(); /* the runtime's last-error slot is sticky: clear it */    \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e__);                      \
            return AZR_E_HIP;                                                                   \
        }                                                                                       \
    } while (0)

// Test hooks.  Environment switches that select an older or alternative formulation of the same arithmetic (the parity tests compare it
// with the default one as an independently written implementation), force a hand-off to give up, or stand in for a communicator exist
// ONLY in libazr_hip_test.so — the same sources compiled with -DAZR_TEST_HOOKS by `make test` (csrc/Makefile), loaded by the tests that
// need them.  The product library libazr_hip.so reads no environment variable and carries one path.
#ifdef AZR_TEST_HOOKS
#include <stdlib.h>
namespace azr {
inline const char* hook_env(const char* name) { return getenv(name); }
}
#else
namespace azr {
constexpr const char* hook_env(const char*) { return nullptr; }
}
#endif
namespace azr {
inline int hook_env_int(const char* name, int dflt) { const char* v = hook_env(name); return v ? atoi(v) : dflt; }

constexpr int LEAF_STRIDE = 96;    // in88 padded to 96 B per game
constexpr int PI_STRIDE = 44;      // pi[43] padded
constexpr int STAGE_BYTES = 264;   // staged record: in88 @0 | pi[43] @88 | player @260
constexpr int NF = 256;            // FILTERS (python/src/build_graph.py:32)
constexpr int NPOS = 42;

// head section of the AZRW vector, in floats from its start: policy 1x1 conv [256][2], its BN g[2] b[2] m[2] v[2],
// policy dense [84][43] + bias [43]; value 1x1 conv [256], its BN g b m v, dense [42][256] + bias [256], output [256] + bias [1]
constexpr int H_PI_W = 0, H_PI_BN = 512, H_PD_W = 520, H_PD_B = 4132, H_V_W = 4175, H_V_BN = 4431, H_V1_W = 4435,
              H_V1_B = 15187, H_V2_W = 15443, H_V2_B = 15699, HEAD_FLOATS = 15700;
static_assert(H_PI_BN == H_PI_W + NF * 2 && H_PD_W == H_PI_BN + 8 && H_PD_B == H_PD_W + 84 * 43 && H_V_W == H_PD_B + 43 &&
              H_V_BN == H_V_W + NF && H_V1_W == H_V_BN + 4 && H_V1_B == H_V1_W + 42 * 256 && H_V2_W == H_V1_B + 256 &&
              H_V2_B == H_V2_W + 256 && HEAD_FLOATS == H_V2_B + 1, "the head section's parts tile it without gaps");

// device view handed to kernels by value
struct Dev {
    int G, C, H, DMAX, SCAP;
    int T;                 // THREADS_PER_MCTS: search threads (= leaf slots) per game; slot = g * T + k
    Rules rules;
    Search search;
    int search2_simulations;   // two-net arena: player AZR_PLAYER_ALPHAZERO_B's simulations per decision and PUCT constant
    float search2_hp;          // (azr_arena_set_opponent_search; the handle's own unless set).  Read by the arena step only.
    uint8_t* state;        // [G][64] game records
    Ctl* ctl;              // [G]
    uint8_t* nodes;        // [G][C][NODE_BYTES]
    uint32_t* touch;       // [G][C]
    uint32_t* nhash;       // [G][C]
    uint32_t* table;       // [G][H]
    uint16_t* freel;       // [G][C]
    uint32_t* path;        // [G][T][DMAX]
    uint8_t* leaf_in;      // [G*T][LEAF_STRIDE]
    uint8_t* leaf_key;     // [G*T][64]
    uint64_t* leaf_valid;  // [G*T]
    uint32_t* leaf_hash;   // [G*T]
    float* net_pi;         // [G*T][PI_STRIDE]
    float* net_v;          // [G*T]
    uint8_t* stage;        // [G][SCAP][STAGE_BYTES]
    uint8_t* ring;         // [RCAP][265]
    unsigned long long* ring_count;
    unsigned long long ring_cap;
    Counters* counters;
    uint32_t* active;      // number of games with a pending leaf after the last tree step
    uint32_t base_seed;
    unsigned long long sp_quota;      // self-play quota mode: games to start in all (0 = unlimited)
    unsigned long long* sp_started;   // ... and the ticket counter
    int sp_compact;                   // self-play tail: the tree step lists the waiting leaf slots (leaf_list[0], leaf_count[0]) and
                                      // the net runs on that list only
    // arena (GameGroup::playGames, game/game.cpp:277-312)
    int kind0, kind1;          // AZR_PLAYER_* of player index 0 / 1
    int arena_total;           // Counter::count
    int arena_slot_cap;        // optional cap of games per slot (0 = none)
    int arena_mirror;          // SETTINGS.MIRROR_GAMES
    int* arena_taken;          // Counter::i
    int* arena_res;            // GameResults: count, draw, win0, winStarted0, win1, winStarted1
    uint8_t* prev_start;       // [G][64]  Game::previousStartState
    uint8_t* script;           // [G][2][32]  ScriptW
    int8_t* alog_status;       // [G][ALOG]
    uint16_t* alog_rounds;     // [G][ALOG]
    uint8_t* alog_final;       // [G][ALOG][64]
    // two-net arena (trainAZPG vs generateAZPG, alphazero_trainer.cpp:147-152): AZR_PLAYER_ALPHAZERO_B searches its own
    // tree (every AlphaZeroPlayer owns an AlphaZeroMCTS) and is evaluated by the opponent handle's network
    uint8_t* nodes2;           // [G][C][NODE_BYTES]   (null until azr_arena_set_opponent_net)
    uint32_t* touch2;
    uint32_t* nhash2;
    uint32_t* table2;
    uint16_t* freel2;
    uint32_t* tctl2;           // [G][4]  tree 2's {search_id, nfree, hiwater, -}
    int* leaf_list;            // [2][G*T] leaf slots waiting for net A / net B after an arena step
    int* leaf_count;           // [2][2]: [0][net] by default; the arena's passes without a read-back alternate between the two rows
    int lc_base;               // ... row (x 2) the arena step counts into
    int lc_zero;               // ... row (x 2) the arena step zeroes for the next pass (nobody reads it any more), or -1
    int arena_collect;         // stage (s, pi, player) per AlphaZero decision and flush finished games to the record ring
    // root noise (this engine's own; read by the k_tree_step instantiations with NOISE only, never by the arena)
    float* root_eta;           // [G][43]  the vector in force at each game's root (lane i <-> move i)
    float noise_eps;           // DIR_NOISE_EPSI: noiseP = c1 * P + noise_eps * eta at path depth 0
    float noise_alpha;         // device self-play: Dirichlet(alpha) per new root ...
    uint32_t noise_seed;       // ... keyed by (noise_seed, game seed, decision, move)
    // playout cap (this engine's own; read by the k_tree_step instantiations with CAP, k_selfplay_noise with CAP or FORCED and
    // k_decision_kind only): decision d of the game with seed s is full iff cap_full(cap_threshold, cap_seed, s, d) (azr_cap.hpp)
    uint32_t cap_threshold;    // (uint32_t)(full_prob * 2^24)
    uint32_t cap_seed;
    int cap_fast;              // descents of a fast decision: fast_simulations - fast_simulations % T
    float noise_value;         // DIR_NOISE_VALUE: every entry of a fast root's vector (the constant form, bit for bit)
    // forced playouts and policy target pruning (this engine's own; read by the k_tree_step instantiations with FORCED,
    // k_selfplay_noise<false, true> and k_pruned_policy only; azr_forced.hpp)
    float forced_k;            // the factor k of nf = sqrt(k * noiseP * sumN) (0 = off)
    int prune;                 // device self-play: a record's pi comes from the pruned counts
    int eta_const;             // host-stepped: no root vector is set, the search runs on the constant one (noise_value)
    // policy surprise weighting of the records (this engine's own; read by the k_tree_step instantiations with SURPRISE only;
    // azr_surprise.hpp)
    float* stage_kl;           // [G][SCAP]  KL(pi || P) of each staged record (allocated by the first azr_selfplay_start* that weights)
    float psw_share;           // the share of a game's record weight handed out by surprise (0 = off)
    float psw_max;             // the cap on one record's weight
    uint32_t psw_seed;         // the copy coin is keyed by (psw_seed, game seed, record)
#ifdef AZR_TEST_HOOKS
    // AZR_TREE_HASH_AND / AZR_TREE_HASH_OR, read when the engine is created: key_hash returns (h & hash_and) | hash_or (azr_tree.hpp)
    uint32_t hash_and, hash_or;
#endif
    // value mix of the records (this engine's own; read by the k_tree_step instantiations with QMIX only; azr_valuemix.hpp).  Behind
    // everything else: the offsets the kernels without it read stay where they were.
    float q_share;             // the share of the root value q in a record's z (0 = off)
    float* stage_q;            // [G][SCAP]  q of each staged record's root, NaN = none (allocated by the first azr_selfplay_start* that blends)
    // resignation with a no-resign holdout (this engine's own; read by the self-play k_tree_step instantiations, once per decision;
    // azr_resign.hpp).  No template argument: resign_streak is wave-uniform, and 0 leaves the step what it was.
    int resign_streak;         // decisions in a row below resign_q after which their player gives up (0 = off)
    float resign_q;            // the bound on the root value q
    uint32_t resign_threshold; // (uint32_t)(holdout_share * 2^24): the holdout coin's
    uint32_t resign_seed;      // the coin is keyed by (resign_seed, game seed)
    uint32_t* resign_state;    // [G]  run[0] | run[1] << 8 | first << 16 of each slot's running game (azr_resign.hpp)
    unsigned long long* resign_stats;   // [G][4]  resigned, holdout_games, holdout_would_resign, holdout_not_lost: per slot, summed by the host
    // Gumbel root search (this engine's own; read by the k_tree_step instantiations with GUMBEL, k_selfplay_gumbel, k_gumbel_policy and
    // k_gumbel_pick only; azr_gumbel.hpp).  Behind everything else again.  Both arrays are allocated at first use.
    float* root_g;             // [G][43]  the Gumbel vector in force at each game's root (lane i <-> move i)
    uint32_t* root_n0;         // [G][43]  N0: the root's N row when the search in progress made its first root-level selection
    int gumbel_m;              // moves considered at a root (0 = off)
    float gumbel_cvisit;       // sigma = ((c_visit + max N) * c_scale) * qhat
    float gumbel_cscale;
    uint32_t gumbel_seed;      // device self-play: g is keyed by (gumbel_seed, game seed, decision, move)
};
// The arena's Gumbel search (azr_arena_set_gumbel): one AlphaZero side's settings, and both sides' as k_arena_step_gumbel takes them —
// a kernel argument of its own behind Dev, which therefore does not grow (a larger Dev would move the trailing arguments of every kernel
// that has some).  side[0] = AZR_PLAYER_ALPHAZERO, side[1] = AZR_PLAYER_ALPHAZERO_B.  g = 0: nothing is drawn.
struct GumbelSide {
    int m = 0;                 // moves considered at a root (0 = off: this side searches by PUCT)
    float c_visit = 0.0f, c_scale = 0.0f;
    int tree = 0;              // 1 = gumbel_select_tree below the root, 0 = PUCT with the side's own hp
};
struct ArenaGumbel { GumbelSide side[2]; };
constexpr int ALOG = 16;

// The options of the search variants (host side).  Which of them a tree step carries: root noise, a playout cap (self-play only),
// forced playouts, policy surprise weighting of the records and the value mix of their z (both self-play only) — the template
// arguments of k_tree_step after SELFPLAY; the Gumbel root search, which excludes the first three; and its selection below the root
// (gtree), which needs it.
struct StepOpts { bool noise = false, cap = false, forced = false, surprise = false, qmix = false, gumbel = false, gtree = false; };
// Host-stepped searches (azr_mcts_*): in force from the setter's call until the next azr_selfplay_start*.
struct HostOpts {
    bool noise = false;        // azr_mcts_set_root_noise: a vector per game is set in d.root_eta
    float forced_k = 0.0f;     // azr_mcts_set_forced_playouts (0 = off)
    int sims = 0;              // azr_mcts_set_simulations: the budget (0 = the settings')
    int gumbel_m = 0;          // azr_mcts_set_gumbel (0 = off)
    float gumbel_cvisit = 0.0f, gumbel_cscale = 0.0f;
    bool gumbel_tree = false;  // azr_mcts_set_gumbel_tree
};
// Device self-play, as the azr_selfplay_set_* setters leave them.  A running self-play never sees a change: azr_selfplay_start* resolves
// them into a StepOpts and Dev's noise_*, cap_*, forced_k, prune, psw_*, q_share, resign_* and gumbel_*.
struct SelfplayOpts {
    float alpha = 0.0f;        // azr_selfplay_set_dirichlet (0 = off)
    uint32_t noise_seed = 0;
    float cap_prob = 1.0f;     // azr_selfplay_set_playout_cap (off: cap_prob >= 1 or cap_fast_sims <= 0)
    int cap_fast_sims = 0;
    uint32_t cap_seed = 0;
    float forced_k = 0.0f;     // azr_selfplay_set_forced_playouts (0 = off)
    bool prune = false;
    float psw_share = 0.0f;    // azr_selfplay_set_surprise_weighting (0 = off)
    float psw_max = 1.0f;
    uint32_t psw_seed = 0;
    float q_share = 0.0f;      // azr_selfplay_set_value_mix (0 = off)
    int resign_streak = 0;     // azr_selfplay_set_resign (0 = off)
    float resign_q = 0.0f;
    float resign_holdout = 0.0f;
    uint32_t resign_seed = 0;
    int gumbel_m = 0;          // azr_selfplay_set_gumbel (0 = off)
    float gumbel_cvisit = 0.0f, gumbel_cscale = 0.0f;
    uint32_t gumbel_seed = 0;
    int gumbel_tree = 0;       // azr_selfplay_set_gumbel_tree (0 = PUCT below the root)
};

// folded network parameters on device
struct NetDev {
    int blocks;
    // fp32 path
    float* stem_w;     // [9][13][256]
    float* stem_scale; // [7] per board row (conv_bn, axis=1)
    float* stem_shift; // [7]
    float* tower_w;    // [2B][9][256][256]
    float* tower_scale;// [2B][256]
    float* tower_shift;// [2B][256]
    float* d_flat;     // whole AZRW vector on device (fp32 conv kernels and the heads read it in place)
    float* d_fold;     // folded BN: stem scale[7] shift[7]; per conv layer scale[256] shift[256]
    const float* head; // head section of d_flat
    // bf16 MFMA path
    void* bf16ctx;      // azr_net_bf16.hip: packed weight fragments + tower output buffer
    void* fxctx;        // azr_tower_fx.hip (AZR_NET_F32X): packed fp16-pair weight fragments
    // azr_nn_predict staging, created by the first call: device [G] x (96 B in | 44 floats pi | 1 float v), the same in pinned host memory
    uint8_t* pred_dev;
    uint8_t* pred_host;
    // activations (fp32 path)
    float* actX;       // [G][42][256]
    float* actT;       // [G][42][256]
};

// the events of one sampled pass of azr_selfplay_run, in stream order: the tree step begins / ends (= the net begins), around the net's
// dominant kernel (pe_tower0 / pe_tower1 below), the net ends
struct ProfEvents {
    hipEvent_t tree0, tree1, net1, tower0, tower1;
};
constexpr int PROF_MAX = 24;   // sampled passes per run

// azr_default_train_options: the reference's graph (build_graph.py:30-31,103) — Adam at a constant 1e-3, L2 1e-3, no clipping, no EMA
constexpr azr_train_options TRAIN_OPT_DEFAULT = {1e-3f, 1e-3f, AZR_LR_CONSTANT, 0, 0, 1, 1.0f, 0.0f, 0.0f, 0.0f};

}  // namespace azr

struct azr_engine {
    azr_settings cfg;
    azr::Dev d;
    azr::NetDev net;
    hipStream_t stream;
    std::string err;
    std::vector<float> flat;      // AZRW host copy
    int mode;                     // 0 rules only / stepwise, 2 self-play
    // profiling of the last azr_selfplay_run: one set of events per sampled pass, created by the first run
    azr::ProfEvents ev[azr::PROF_MAX] = {};
    float prof_net_ms, prof_tree_ms, prof_tower_ms;
    hipEvent_t pe_tower0 = nullptr, pe_tower1 = nullptr;  // when set, the net records these around its dominant kernel
    int prof_launches;
    bool weights_set;
    void* tree2[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // nodes2, touch2, nhash2, table2, freel2, tctl2
    azr_engine* opponent = nullptr;  // handle whose network plays AZR_PLAYER_ALPHAZERO_B (azr_arena_set_opponent_net)
    unsigned arena_pass = 0;         // passes of the running arena that were queued without a read-back (parity = leaf_count row)
    hipEvent_t arena_ev2 = nullptr;  // ... and this stream's tree step done -> the opponent's net launch may start
    hipEvent_t arena_ev = nullptr;   // two-net arena: the opponent's net launch (on ITS stream) done -> this stream may go on
    bool arena_script = false;    // azr_arena_collect_scripted_samples
    bool arena_rec = false;       // ... as azr_arena_start found it: this arena's steps run k_arena_step_rec
    bool arena_open = false;      // between azr_arena_start and the azr_arena_run that found every slot idle
    int opp_simulations = -1;     // azr_arena_set_opponent_search: player B's count per decision and PUCT constant (< 0 = the handle's own);
    float opp_hp = -1.0f;         // copied into d.search2_* by azr_arena_start
    azr::ArenaGumbel arena_gumbel_set;   // azr_arena_set_gumbel, as it stands ...
    azr::ArenaGumbel arena_gumbel_run;   // ... and as azr_arena_start found it: a running arena never sees a change
    bool arena_gumbel = false;    // a side of this arena has m > 0: its steps run k_arena_step_gumbel(d, arena_gumbel_run)
    azr::HostOpts host;           // the host-stepped options as they stand
    azr::SelfplayOpts sp_set;     // the self-play options as set ...
    azr::StepOpts sp;             // ... and what azr_selfplay_start* found in force: this self-play's steps carry it (the values are in d)
    bool sp_tail = false;         // quota self-play: no game is left to start, slots go idle -> compacted net batches
    void* train = nullptr;        // azr_train.hip: optimiser state + activation slabs, created by the first azr_nn_train*
    // azr_nn_train_set_options: on the handle, not in the training context — a reset, a rebuild and a failed health check leave them
    azr_train_options train_opt = azr::TRAIN_OPT_DEFAULT;
    void* dp_comm = nullptr;      // azr_dp_init: this handle's RCCL communicator (ncclComm_t), rank and world
    int dp_rank = 0, dp_world = 0;
};

namespace azr {
// net (azr_net.hip)
int net_alloc(azr_engine* h);
void net_free(azr_engine* h);
int net_upload(azr_engine* h);  // fold BN, pack, copy h->flat to the device
int net_forward(azr_engine* h, const uint8_t* d_in88, int in_stride, int n, float* d_pi, float* d_v);
int net_forward_ex(azr_engine* h, const uint8_t* d_in88, int in_stride, int n, float* d_pi, float* d_v, const int* d_map, hipStream_t st);
bool net_forward_counted_ok(azr_engine* h, int n_max);
int net_forward_counted(azr_engine* h, const uint8_t* d_in88, int in_stride, int n_max, const int* n_dev, const int* n_other, int other_wgpp, float* d_pi, float* d_v, const int* d_map, hipStream_t st);
int net_counted_wgs_per_pair(azr_engine* h);   // what a split-channel launch beside h's counted launch charges a board pair of h's with
size_t net_param_count(int blocks);
void net_init_random(float* flat, int blocks, uint64_t seed);
int net_fallbacks(azr_engine* h, unsigned long long* out);   // split-channel tower launches recomputed after a hand-off gave up
// NET_F32X (azr_tower_fx.hip)
int net_fx_alloc(azr_engine* h);
void net_fx_free(azr_engine* h);
int net_fx_upload(azr_engine* h, const float* fold_host);
int net_fx_forward(azr_engine* h, const uint8_t* d_in88, int in_stride, int n, float* d_pi, float* d_v, const int* d_map, hipStream_t st);
bool net_fx_counted_ok(azr_engine* h, int n_max);
int net_fx_forward_counted(azr_engine* h, const uint8_t* d_in88, int in_stride, int n_max, const int* n_dev, float* d_pi, float* d_v, const int* d_map, hipStream_t st);
// train (azr_train.hip)
void train_free(azr_engine* h);
void dp_free(azr_engine* h);
}  // namespace azr
