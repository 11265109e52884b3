/* azr.h — C-ABI of the MI355X-native AlphaZero-Risk self-play hot path (libazr_hip.so).
 *
 * Drop-in boundary for the reference's three in-process seams (citations relative to the
 * reference tree).  The reference has no FFI; these entry points are what a binding for each seam
 * would call, batched over G concurrent games (one handle = one GPU = one HIP stream set; a handle is
 * NOT re-entrant, different handles are independent — the reference's "one self-play thread per GPU",
 * player/alpha_zero/alphazero_trainer.cpp:48-57).
 *
 * Conventions: every function returns 0 on success or an AZR_E_* code (no exceptions cross the ABI);
 * the caller owns every buffer; `*_host` pointers are host memory, copied through pinned staging;
 * byte images use the reference's own layouts:
 *     state  = `struct Data`            160 B  (state/state.h:86-105)
 *     in88   = `class NNInputData`       88 B  (neural_network/alphazero_nn_data.h:66-96)
 *     rec265 = on-disk training record  265 B  (alphazero_nn_data.cpp:123-130: i8 player | in88 | f32 z | f32 pi[43])
 * Policy index 0..41 = land, 42 = SKIP (land/land.cpp:312), 43 = None.
 */
#ifndef AZR_H
#define AZR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AZR_LANDS 42
#define AZR_MOVES 43
#define AZR_STATE_BYTES 160
#define AZR_INPUT_BYTES 88
#define AZR_RECORD_BYTES 265

enum {
    AZR_OK = 0,
    AZR_E_INVALID_ARGUMENT = 1, /* std::invalid_argument in the reference (illegal phase/move) */
    AZR_E_LOGIC = 2,            /* std::logic_error (army overflow, skip in a non-skippable phase) */
    AZR_E_BAD_HANDLE = 3,
    AZR_E_HIP = 4,              /* a HIP runtime call failed (TF_CHECK_OK abort in the reference) */
    AZR_E_CAPACITY = 5,         /* node pool / path stack / sample buffer exhausted */
    AZR_E_IO = 6,
    AZR_E_STATE = 7             /* call not valid in the engine's current mode */
};

/* arithmetic of the policy/value net contractions.
 *   AZR_NET_BF16  bf16 operands on the MFMA, fp32 accumulate: the fast path (|d pi|, |d v| <= 2e-2 of an fp32 evaluation)
 *   AZR_NET_F32   fp32 on the vector ALU: the precise, slow path (tolerance anchor of the tests)
 *   AZR_NET_F32X  fp32-equivalent on the MFMA: every conv operand as an fp16 pair (22 significand bits), three MFMA passes
 *                 per layer, fp32 accumulate / epilogue / residual / heads — the reference evaluates in fp32
 *                 (alphazero_nn.cpp:247-248); <= 2e-5 of the fp32 evaluation.  Conv weights must lie in the fp16 range.
 *   AZR_NET_F16   fp16 operands on the MFMA (the kernels and the rate of AZR_NET_BF16, 11 significand bits instead of 8): ~7x
 *                 closer to the fp32 evaluation than bf16 (<= 3e-3).  Conv weights must lie in the fp16 range (they are packed
 *                 as 2^k w per layer); activations saturate at 65504. */
enum { AZR_NET_F32 = 0, AZR_NET_BF16 = 1, AZR_NET_F32X = 2, AZR_NET_F16 = 3 };

/* Mirrors the fields of `class Settings` the hot path reads (src/settings.h:41-64) + engine sizing. */
typedef struct azr_settings {
    int32_t device;                /* HIP device ordinal */
    int32_t games;                 /* G: concurrent games on this handle (gpu-games, settings.h:163-171) */
    int32_t blocks;                /* residual blocks B (CMakeLists.txt:15 BLOCKS, 20) */
    int32_t net_dtype;             /* AZR_NET_F32 | AZR_NET_BF16 | AZR_NET_F32X | AZR_NET_F16 */
    int32_t mcts_simulations;      /* MCTS_SIMULATIONS (--mcts) */
    int32_t mcts_threads;          /* THREADS_PER_MCTS (-t, settings.h:44; default 2): T lock-stepped search threads per
                                      game with the reference's active_N virtual loss; 1..8.  Leaf slots = games * T. */
    int32_t allow_yield;           /* ALLOW_YIELD (--allow-yield) */
    int32_t limit_reinforcement;   /* LIMIT_REINFORCEMENT_MOVES (--limit-reinforcement) */
    int32_t limit_attack;          /* LIMIT_ATTACK_MOVES (--limit-attack) */
    int32_t max_game_rounds;       /* MAX_GAME_ROUNDS 58 */
    int32_t min_unit_move;         /* MIN_UNIT_MOVE 3 */
    int32_t temperature_threshold; /* TEMPERATURE_TRESHOLD (--temp) */
    float hp_exploration;          /* HP_EXPLORATION (--hp) */
    float dir_noise_value;         /* DIR_NOISE_VALUE (--dnv) */
    float dir_noise_epsi;          /* DIR_NOISE_EPSI (--dne) */
    int32_t node_capacity;         /* tree nodes per game; 0 = 16 * (mcts_simulations + 1); at least 8 are allocated.  A full pool
                                      never stops a search: a leaf that finds it full is not stored (its value is still backed up,
                                      and a later descent asks for it again); a ROOT that finds it full after the trim empties the
                                      tree, as clearNodes does, and is placed.  Both are counted in nodes_dropped. */
    int32_t sample_capacity;       /* (s,pi,z) records buffered per game before a drain; 0 = 4096 */
} azr_settings;

typedef struct azr_engine azr_engine;

/* Settings() defaults (src/settings.h:22-81) */
void azr_default_settings(azr_settings* s);

/* On failure *out is NULL, nothing stays allocated and azr_last_error(NULL) holds the calling thread's reason.
 * AZR_E_INVALID_ARGUMENT also for a node pool (node_capacity, or the default 16 * (mcts_simulations + 1)) above the
 * 65534 nodes per game a 16-bit node index addresses. */
int azr_engine_create(const azr_settings* s, azr_engine** out);
int azr_engine_destroy(azr_engine* h);
const char* azr_last_error(const azr_engine* h);   /* h == NULL: the last failed azr_engine_create of this thread */
int azr_engine_games(const azr_engine* h);

/* ---- game rules: `class State` + UtilityNN (state/state.cpp, alphazero_moves.cpp) -------------------- */
/* State::newGame (state.cpp:137-167) for game g with its own minstd_rand0 stream seeded seeds[g]
 * (replaces the reference's process-global RNG, src/rng.h:50). */
int azr_engine_new_games(azr_engine* h, const uint32_t* seeds_host);
int azr_engine_set_states(azr_engine* h, const void* data160_host); /* [G][160] */
int azr_engine_get_states(azr_engine* h, void* data160_host);       /* [G][160], padding bytes zero */
int azr_engine_set_rng(azr_engine* h, const uint32_t* engine_state_host); /* raw minstd_rand0 state per game */
int azr_engine_get_rng(azr_engine* h, uint32_t* engine_state_host);
/* UtilityNN::getValidMoves (alphazero_moves.cpp:3-70): bit i = land i, bit 42 = SKIP */
int azr_engine_valid_moves(azr_engine* h, uint64_t* masks_host);
/* UtilityNN::makeMove (alphazero_moves.cpp:72-233); rc_host[g] (optional) = AZR_OK / AZR_E_INVALID_ARGUMENT /
 * AZR_E_LOGIC per game, as the reference's throw sites; moves_host[g] = 255 leaves game g untouched. */
int azr_engine_make_moves(azr_engine* h, const uint8_t* moves_host, uint8_t* rc_host);
/* State::gameStatus (state.cpp:518-565): -1 running, 0/1 winner, -2 draw */
int azr_engine_status(azr_engine* h, int8_t* status_host);
/* NNInputData(const State&) (alphazero_nn_data.cpp:165-196) */
int azr_engine_encode(azr_engine* h, void* in88_host); /* [G][88] */

/* ---- NN service: AlphaZeroNNId (alphazero_gpu_cluster.h:14-47) ------------------------------------------ */
size_t azr_nn_param_count(int blocks);                     /* floats in the AZRW flat vector */
int azr_nn_init_random(azr_engine* h, uint64_t seed);      /* `init` op: Glorot-uniform kernels, BN identity */
int azr_nn_set_weights(azr_engine* h, const float* flat_host, size_t count);
int azr_nn_get_weights(azr_engine* h, float* flat_host, size_t count);
int azr_nn_load(azr_engine* h, const char* path);          /* loadCheckpoint (alphazero_nn.cpp:189-204) */
int azr_nn_save(azr_engine* h, const char* path);          /* saveCheckpoint (alphazero_nn.cpp:206-214) */
/* predict / processBatchPrediction (alphazero_nn.cpp:236-267,322-349): n inputs -> softmax pi[n][43], tanh v[n] */
int azr_nn_predict(azr_engine* h, const void* in88_host, int n, float* pi_host, float* v_host);
/* AlphaZeroNN::train (alphazero_nn.cpp:351-410) on n 265-byte records: per epoch shuffle (std::shuffle with a
 * minstd_rand0 — *shuffle_rng_state is the raw engine state in and out, standing in for the process-global RNG,
 * src/rng.h:50; NULL = default-seeded), floor(n / batch_size) minibatch steps of the `optimize` op (fp32 forward in
 * training mode, loss, backward, Adam; python/src/build_graph.py:54-103), remainder dropped.  loss_*_host[e] = the
 * epoch averages the reference prints and logs (NaN when n < batch_size).  Adam moments and step count persist on the
 * handle across calls like the TF session's slots; inference weights are refolded / repacked before returning.
 * Range: the forward conv multiplies fp16 pairs of 2^10 w, so a conv weight with |w| >= 64 (or a weight that is not a number) cannot be
 * represented; that, and a loss that stops being a number, is detected behind every epoch: the call then returns
 * AZR_E_INVALID_ARGUMENT with the reason in azr_last_error, the handle's weights are those from before the call and its optimiser
 * state is dropped (the reference's TensorFlow step would carry the NaNs on silently). */
int azr_nn_train(azr_engine* h, const void* rec265_host, size_t n, int epochs, int batch_size,
                 uint32_t* shuffle_rng_state, float* loss_pi_host, float* loss_v_host);
/* the validation phase of AlphaZeroNN::trainCrossValidation (alphazero_nn.cpp:512-548): floor(n / batch_size) batches of
 * records in the given order, forward in inference mode (BN on the moving statistics), no update.  *loss_*_out = the float
 * sum of the batch means divided by the batch count (NaN when n < batch_size, as the reference's 0 / 0); rec_*_host
 * (optional) = per-record cross-entropy / squared error of the batches * batch_size evaluated records.
 * The pass runs at the training step's precision whatever the handle's inference dtype, and changes nothing on the handle:
 * weights, moving statistics, Adam moments and step count stay as they are.  Errors as azr_nn_train (AZR_E_STATE without
 * weights, AZR_E_INVALID_ARGUMENT for batch_size < 2, NULL records with n > 0, or a conv weight outside the fp16-pair range). */
int azr_nn_validate(azr_engine* h, const void* rec265_host, size_t n, int batch_size,
                    float* loss_pi_out, float* loss_v_out, float* rec_loss_pi_host, float* rec_loss_v_host);
/* Data-parallel AlphaZeroNN::train: the same epochs / shuffles / minibatches, every minibatch split over `world` ranks
 * (one process per GPU; the reference trains on GPU 0 only and hands the weights over through checkpoints/temp.bin,
 * alphazero_gpu_cluster.cpp:221-231).  Every rank passes ALL n records and the same *shuffle_rng_state and takes slice
 * `rank` of each minibatch (batch_size % world == 0).  Whatever spans the minibatch — batch-norm statistics in the
 * forward pass, their two sums in the backward pass, the losses, and at the end of the step the whole gradient vector
 * (azr_nn_param_count floats) — is summed over the ranks through `allreduce`: in place on DEVICE memory of this GPU,
 * dtype 0 = float32, 1 = float64, return 0 on success; the engine's stream is idle while it runs.  All ranks then take the
 * same Adam step, so their weights stay equal without a broadcast, and equal the single-GPU step's up to summation
 * order.  world = 1 with allreduce == NULL and no communicator is azr_nn_train; world = 1 WITH a callback (or a one-rank
 * communicator, azr_dp_init) runs the data-parallel code path on one rank (every all-reduce is the identity): the single-GPU
 * rehearsal of the RCCL path.  allreduce == NULL with world > 1 needs azr_dp_init(h, rank, world, ...). */
typedef int (*azr_allreduce_fn)(void* ctx, void* device_ptr, size_t count, int dtype);
int azr_nn_train_dp(azr_engine* h, const void* rec265_host, size_t n, int epochs, int batch_size, uint32_t* shuffle_rng_state,
                    int rank, int world, azr_allreduce_fn allreduce, void* ctx, float* loss_pi_host, float* loss_v_host);
/* The handle's own RCCL communicator for azr_nn_train_dp (one process per GPU, RCCL over xGMI).  With it — and allreduce == NULL —
 * every sum of the data-parallel step is an ncclAllReduce on the engine's own stream: stream-ordered, no host hand-over (2B + 6
 * small sums and one of azr_nn_param_count floats per step).  Rank 0 draws the 128-byte id (azr_dp_unique_id) and passes it to the
 * other processes by whatever the launcher offers (torch.distributed broadcast, MPI, a file); then EVERY rank calls azr_dp_init
 * (collective).  RCCL is bound at run time ("librccl.so.1": the copy already loaded into the process, else /opt/rocm's);
 * AZR_E_STATE if there is none.  azr_engine_destroy shuts the communicator down. */
#define AZR_DP_ID_BYTES 128
int azr_dp_unique_id(void* id128);
int azr_dp_init(azr_engine* h, int rank, int world, const void* id128);
int azr_dp_shutdown(azr_engine* h);
/* one `session->Run(..., {optimize})` (alphazero_nn.cpp:389-391) on exactly n records in the given order */
int azr_nn_train_batch(azr_engine* h, const void* rec265_host, int n, float* loss_pi, float* loss_v);
/* diagnostics: gradient vector of the last step in AZRW layout (moving-statistics slots unused): the last STEP's, whatever was
 * rebuilt since */
int azr_nn_train_grads(azr_engine* h, float* flat_host, size_t count);
/* drop the optimiser state and the training buffers */
int azr_nn_train_reset(azr_engine* h);
/* Options of the optimiser step: learning-rate schedule, global-norm gradient clipping, an exponential moving average (EMA) of the
 * weights.  The defaults are the reference's graph (build_graph.py: Adam at a constant 1e-3, L2 1e-3, nothing else), and with every
 * option at its default the step launches the kernels it launched before the options existed.
 * Lifetime: the options live on the handle — they survive azr_nn_train_reset, a rebuild of the training context and a failed health
 * check — and are read once when azr_nn_train, azr_nn_train_dp or azr_nn_train_batch is entered; a running call never sees a setter.
 * Schedule: evaluated on the device, in double, from Adam's step count t (1-based behind the increment; azr_nn_train_reset restarts it
 * at 0), so azr_nn_train's queue of steps needs no host round trip:
 *   warm(t) = W > 0 ? min(1, t / W) : 1                                         (W = warmup_steps)
 *   CONSTANT: f = 1
 *   COSINE:   p = clamp((t - W) / (N - W), 0, 1), f = r + (1 - r) * 0.5 * (1 + cos(pi * p)), r = lr_min / lr     (N = total_steps)
 *   STEP:     f = decay_gamma ^ floor((t - 1) / decay_period)
 *   lr_eff = lr * warm * f,   lr_t = (float)(lr_eff * sqrt(1 - b2^t) / (1 - b1^t))    (the bias-corrected rate Adam multiplies by)
 * Clipping (tf.clip_by_global_norm on the gradient of the whole loss): g^ = g + 2 * l2 * w on the conv / dense kernels, g^ = g on BN
 * gamma / beta and biases, the BN moving statistics take no part; norm = sqrt(sum g^2), s = clip_norm / max(norm, clip_norm), Adam
 * sees s * g^.  The sum is in double, atomic-free and in a fixed order: two runs give the same bits, and under azr_nn_train_dp it
 * runs behind the gradient all-reduce, so every rank computes the same bits.  azr_nn_train_grads keeps returning the raw g.
 * EMA: the first step taken with ema_decay = d > 0 creates the vector as a copy of the weights from before that step; every step
 * then sets e = d * e + (1 - d) * w_new on the trained slots and e = w_new on the BN moving statistics (averages already).  The
 * vector is optimiser state: it lives through a rebuild of the training context as Adam's moments do, and azr_nn_train_reset and a
 * failed health check drop it.  azr_nn_get_ema_weights returns it as an AZRW vector that azr_nn_set_weights accepts on any handle.
 * azr_nn_train_set_options: AZR_E_INVALID_ARGUMENT, with a reason in azr_last_error and the previous options still in place, for a
 * value that is not finite, lr <= 0, l2 < 0, an unknown schedule, warmup_steps < 0, COSINE with total_steps <= warmup_steps or lr_min
 * outside [0, lr], STEP with decay_period < 1 or decay_gamma outside (0, 1], clip_norm < 0, ema_decay outside [0, 1). */
enum { AZR_LR_CONSTANT = 0, AZR_LR_COSINE = 1, AZR_LR_STEP = 2 };
typedef struct azr_train_options {
    float   lr;            /* base learning rate, default 1e-3f (build_graph.py) */
    float   l2;            /* L2 coefficient of the conv / dense kernels, default 1e-3f */
    int32_t lr_schedule;   /* AZR_LR_*, default CONSTANT */
    int32_t warmup_steps;  /* W >= 0, default 0 */
    int32_t total_steps;   /* COSINE: N > W, the step at which lr_min is reached */
    int32_t decay_period;  /* STEP: every so many steps ... (>= 1, default 1) */
    float   decay_gamma;   /* ... the rate is multiplied by gamma, in (0, 1], default 1 */
    float   lr_min;        /* COSINE floor, in [0, lr] */
    float   clip_norm;     /* global-norm clipping, 0 = off, else > 0 */
    float   ema_decay;     /* d in (0, 1), 0 = off */
} azr_train_options;
typedef struct azr_train_stats {   /* of the LAST step taken on the handle */
    int64_t step;          /* Adam step count t */
    float   lr, lr_t;      /* scheduled rate, and the bias-corrected rate Adam used */
    float   grad_norm;     /* NaN where it was not computed (clipping off) */
    float   clip_scale;    /* 1 where nothing was clipped */
    int64_t clipped_steps; /* steps with clip_scale < 1 since the optimiser state was created */
    int64_t ema_steps;     /* steps folded into the EMA vector */
} azr_train_stats;
void azr_default_train_options(azr_train_options* o);
int azr_nn_train_set_options(azr_engine* h, const azr_train_options* o);
int azr_nn_train_get_options(azr_engine* h, azr_train_options* o);
/* AZR_E_STATE before the first step (and behind azr_nn_train_reset or a failed health check) */
int azr_nn_train_stats(azr_engine* h, azr_train_stats* out);
/* AZR_E_STATE while there is no EMA vector; count = azr_nn_param_count */
int azr_nn_get_ema_weights(azr_engine* h, float* flat_host, size_t count);

/* ---- search: AlphaZeroMCTS / StateSimulationsStorage (alphazero_mcts.h:55-95) ---------------------------- */
int azr_mcts_clear(azr_engine* h);   /* clearNodes (alphazero_mcts.cpp:223-227), all games */
int azr_mcts_trim(azr_engine* h);    /* trimNodes  (alphazero_mcts.cpp:229-245), all games */
/* AlphaZeroMCTS::simulate (alphazero_mcts.cpp:255-307) for all G roots in lock-step: trim, expand the root if unknown,
 * then mcts_simulations - mcts_simulations % mcts_threads searches per game by mcts_threads search threads that block
 * together at the NN seam (thread k of game g = leaf slot g * T + k; threads run in index order — one of the
 * reference's possible schedules, and the only one at T = 1).  Finished games idle. */
int azr_mcts_simulate(azr_engine* h);
/* The same search split at the NN seam (predictFuture, alphazero_mcts.cpp:350-351), so a caller can supply
 * priors/values itself: begin -> { leaves -> [evaluate] -> apply }* until *active_out == 0. */
int azr_mcts_begin(azr_engine* h);
/* in88_host [G*T][88], need_eval_host [G*T], pi_host [G*T][43], v_host [G*T]; slot = g * T + k */
int azr_mcts_leaves(azr_engine* h, void* in88_host, uint8_t* need_eval_host, int* active_out);
int azr_mcts_apply(azr_engine* h, const float* pi_host, const float* v_host);
/* root statistics of the last search: N[G][43]; Q,P optional */
int azr_mcts_root_stats(azr_engine* h, uint32_t* n_host, float* q_host, float* p_host);
/* The rows of any node of a game's tree: state g of data160_host [G][160] is imported as azr_engine_set_states imports it, into
 * registers only, and looked up in game g's tree.  n_host = the completed visits, act_host (optional) = the visits in flight, q_host,
 * p_host [G][43]; vhat_host [G] (optional) = the net's value kept by a Gumbel search (0 in a node any other search expanded);
 * found_host [G] = 1 where the state is in the tree, else 0 with zero rows.  Read-only: the games' states, the search's bookkeeping and
 * the nodes stay as they are, so it is valid between azr_mcts_leaves and azr_mcts_apply too.  For a game's own current state it returns
 * azr_mcts_root_stats' numbers. */
int azr_mcts_node_stats(azr_engine* h, const void* data160_host, uint32_t* n_host, uint32_t* act_host /*optional*/, float* q_host,
                        float* p_host, float* vhat_host /*optional*/, uint8_t* found_host);
/* StateSimulations::calculateMoveProbability(1.0f) (alphazero_mcts.cpp:121-149) */
int azr_mcts_policy(azr_engine* h, float* pi_host);
/* pickHigestWeightedMove / pickRandomWeightedMove (alphazero_mcts.cpp:379-412) on the last search's policy;
 * sample != 0 draws with the game's own RNG stream (one rFloat). */
int azr_mcts_pick(azr_engine* h, int sample, uint8_t* moves_host);

/* ---- root noise (this engine's own; the default is the reference's constant) ----------------------------------------
 * The reference mixes the constant DIR_NOISE_EPSI * DIR_NOISE_VALUE into every prior at every node (alphazero_mcts.cpp:81) and
 * samples nothing; that is the state after azr_engine_create.  With a noise vector eta in force for a game, the FIRST selection of
 * every descent of that game's search threads (path depth 0) scores move m with
 *     noiseP = (1 - DIR_NOISE_EPSI) * P[m] + DIR_NOISE_EPSI * eta[m]
 * in place of ... + DIR_NOISE_EPSI * DIR_NOISE_VALUE; every deeper level keeps the constant.  eta[m] = DIR_NOISE_VALUE for all m is
 * the constant form bit for bit.  The stored priors, azr_mcts_root_stats, the policies and the records do not change meaning.
 * The arena (azr_arena_*, both trees) never uses root noise: evaluation games are played without it.
 *
 * host-stepped searches (azr_mcts_simulate / azr_mcts_begin..apply): eta_host [G][43] used as given (no masking, no
 * normalising) at path depth 0; NULL = off (the state after create).  Holds until set again; azr_selfplay_start* ends it (the
 * vector array is then the self-play's), and setting it ends a running self-play. */
int azr_mcts_set_root_noise(azr_engine* h, const float* eta_host);
/* device self-play (azr_selfplay_start*): alpha > 0 draws Dirichlet(alpha) over each new root's legal moves;
 * alpha <= 0 = off (default).  Read by azr_selfplay_start*; a running self-play never sees a change.  Every decision's root — the
 * first of a game, the next after a move with the tree's N / Q carried over — gets a new vector, shared by the game's search
 * threads.  The vector for decision d of the game with seed s is a function of (noise_seed, s, d, move, alpha) alone: not of the
 * slot, the number of games or threads, or the pass schedule; nothing is drawn from the game's own RNG stream, so dice, deals
 * and sampled moves are the ones the same search results give without noise.  AZR_E_INVALID_ARGUMENT for a NaN alpha or alpha > 10. */
int azr_selfplay_set_dirichlet(azr_engine* h, float alpha, uint32_t noise_seed);
/* the vector in force at each game's current root, [G][43], zeros where none */
int azr_mcts_root_noise(azr_engine* h, float* eta_host);
/* the sampler alone: n vectors for (game_seed[i], decision[i], valid[i]) -> eta_out [n][43]; valid = legal-move mask as
 * azr_engine_valid_moves; alpha in (0, 10] */
int azr_debug_root_noise(azr_engine* h, float alpha, uint32_t noise_seed, const uint32_t* game_seed,
                         const uint32_t* decision, const uint64_t* valid, int n, float* eta_out);

/* ---- playout cap randomisation in device self-play (this engine's own; off after azr_engine_create) -----------------
 * The reference spends MCTS_SIMULATIONS on every decision of a self-play game and records every decision.  With a cap in force
 * each decision is FULL or FAST by a coin:
 *
 * The coin.  d = the number of decisions already taken in the running game (0 at a game's first decision, and 0 again where
 * azr_selfplay_start_from_states enters a game); s = the game's seed.  All arithmetic is uint32:
 *     mix(x):  x ^= x >> 16;  x *= 0x7FEB352D;  x ^= x >> 15;  x *= 0x846CA68B;  x ^= x >> 16
 *     k = mix(cap_seed + 0xC2B2AE35);   k = mix(k ^ s);   k = mix((k ^ d) + 0x27D4EB2F)
 *     full  <=>  (k >> 8) < (uint32_t)(full_prob * 16777216.0f)          (the threshold is computed once on the host, in float)
 * otherwise the decision is fast.  The coin is a function of (cap_seed, s, d, full_prob) alone: not of the slot, the number of games
 * or threads, the pass schedule, the noise seed or the game's own RNG stream, from which nothing is drawn.  Its domain constants are
 * not the Dirichlet sampler's, so equal seeds do not correlate coin and noise.
 *
 * A full decision is the decision without a cap, exactly: S = mcts_simulations - mcts_simulations % mcts_threads descents, the
 * Dirichlet vector at path depth 0 if azr_selfplay_set_dirichlet is in force, one (s, pi, z) record staged.
 * A fast decision runs F = fast_simulations - fast_simulations % mcts_threads descents; with azr_selfplay_set_dirichlet in force its
 * root vector is the constant eta[m] = DIR_NOISE_VALUE for all 43 entries — the constant form bit for bit (see above) — which is what
 * the engine stores for that root and what azr_mcts_root_noise reports as the vector in force; and it stages NO record.
 * Everything else is the same for both kinds: trim and tree reuse between decisions, the temperature pick against
 * temperature_threshold including its one rFloat, the move, game turnover, quota tickets, and the z back-fill of the staged records
 * when the game ends (every record's z comes from a game played with real searches throughout).
 * Counters: decisions and simulations count both kinds; samples counts written records only.
 * The arena (azr_arena_*) and the host-stepped searches (azr_mcts_*) never see the cap.
 *
 * Read by azr_selfplay_start*; a running self-play never sees a change.  Off (the state after create) for full_prob >= 1 or
 * fast_simulations <= 0.  full_prob == 0 is legal: no decision is full and no record is written.  AZR_E_INVALID_ARGUMENT, with a
 * reason in azr_last_error, for a NaN or negative full_prob, or — when the cap is on — a fast_simulations outside
 * [mcts_threads, mcts_simulations].  The node pool is sized for the full budget. */
int azr_selfplay_set_playout_cap(azr_engine* h, float full_prob, int fast_simulations, uint32_t cap_seed);
/* the kind of each slot's current decision, full_host [G]: 1 = full, 0 = fast.  All 1 when no cap is in force or the engine is not
 * in self-play; 1 for a slot that has gone idle. */
int azr_selfplay_decision_kind(azr_engine* h, uint8_t* full_host);
/* the coin alone, on the device: full_out[i] = 1 / 0 for (game_seed[i], decision[i]), i < n; full_prob >= 0 (>= 1: all full) */
int azr_debug_playout_cap(azr_engine* h, float full_prob, uint32_t cap_seed, const uint32_t* game_seed,
                          const uint32_t* decision, int n, uint8_t* full_out);

/* ---- forced playouts and policy target pruning at the root (this engine's own; off after azr_engine_create) ---------
 * The reference has neither.  Both follow KataGo (Wu 2019, section 3.2) and exist to make sampled root noise worth having: a noised
 * root move is tried often enough for its value to be known, and the visits spent that way do not reach the recorded pi.
 * All arithmetic below is fp32, each operation rounded on its own (no fused multiply-add), in the order written.
 *
 * noiseP[m] is the root-level noised prior of the selection: (1 - DIR_NOISE_EPSI) * P[m] + DIR_NOISE_EPSI * eta[m] with a root
 * vector in force (see "root noise"), (1 - DIR_NOISE_EPSI) * P[m] + DIR_NOISE_EPSI * DIR_NOISE_VALUE otherwise — the same number as
 * eta[m] = DIR_NOISE_VALUE gives.  sumN is the root node's visit total as the selection reads it, N[m] the completed visits of
 * move m (visits in flight in other search threads are not counted, as in the PUCT term).
 *     nf[m] = sqrt((k * noiseP[m]) * (float)sumN)
 *
 * Forced playouts, factor k > 0.  At the FIRST selection of a descent (path depth 0) a legal move m is forced iff N[m] > 0 and
 * (float)N[m] < nf[m].  If at least one move is forced, the selection runs over the forced moves alone — same score, same strict
 * maximum, same tie rule, same bookkeeping; if none is, it is the selection without the feature, bit for bit.  Deeper levels never
 * force.  A root that carries visits over from the previous decision's tree is under the rule from its first descent.
 *
 * Policy target pruning.  With v[m] = (noiseP[m] * hp_exploration) * sqrt(1 + (float)sumN) and sumN, N, Q as the finished search
 * left them:
 *   1. c* = the legal move with the largest N, the lowest index on ties;  U* = Q[c*] + v[c*] / (1 + (float)N[c*]).
 *   2. for every other legal m with N[m] > 0:  f = (uint32)nf[m] truncated (0 where nf is not a positive number);
 *      lower = N[m] > f ? N[m] - f : 0;  N' = N[m];
 *      while (N' > lower  &&  Q[m] + v[m] / (1 + (float)(N' - 1)) < U*)  N' -= 1;
 *      if (N' == 1 && N' < N[m])  N' = 0;                      (a child reduced to a single playout is pruned outright)
 *   3. N'[c*] = N[c*]; a move with N[m] == 0 keeps 0.
 *   4. the pruned policy is azr_mcts_policy's formula on N'.
 * The MOVE of a decision is always picked from the unpruned N: a search with pruning on plays the same games with the same RNG
 * streams and the same z as with pruning off; only pi (bytes 93..264) of its records differs.
 *
 * With a playout cap: a fast decision never forces (and writes no record, so has nothing to prune); a full one forces and prunes.
 * The arena (azr_arena_*) never sees either.
 *
 * host-stepped searches: k <= 0 = off.  Holds until set again; azr_selfplay_start* ends it. */
int azr_mcts_set_forced_playouts(azr_engine* h, float k);
/* the pruned policy pi_host [G][43] and, if not NULL, N' n_pruned_host [G][43] of the last search's roots, under the factor and the
 * root vector in force (a running self-play's, else the host-stepped ones); no factor in force: N' = N.  azr_mcts_policy stays the
 * unpruned policy. */
int azr_mcts_pruned_policy(azr_engine* h, float* pi_host, uint32_t* n_pruned_host);
/* device self-play: k > 0 forces playouts in every full decision; prune != 0 also writes the pruned policy into the records.
 * k <= 0 = off (default).  Read by azr_selfplay_start*; a running self-play never sees a change.  prune != 0 with k <= 0 is an
 * error.  Every setter: AZR_E_INVALID_ARGUMENT, with a reason in azr_last_error, for a NaN k or k > 8. */
int azr_selfplay_set_forced_playouts(azr_engine* h, float k, int prune);
/* the budget of host-stepped searches (azr_mcts_simulate / azr_mcts_begin..apply), so that a caller can retrace a capped self-play
 * decision by decision: simulations in [mcts_threads, mcts_simulations] (S - S % mcts_threads descents), <= 0 = the settings' own
 * (default).  Holds until set again; azr_selfplay_start* ends it.  The arena and device self-play never see it. */
int azr_mcts_set_simulations(azr_engine* h, int simulations);

/* ---- policy surprise weighting of the self-play records (this engine's own; off after azr_engine_create) -------------
 * The reference writes every recorded decision of a finished game once.  With surprise weighting (KataGo, KataGoMethods.md) a game's
 * total record weight stays its record count n, but a share of it is handed out in proportion to KL(pi || P) — the recorded search
 * policy against the net's prior at that root — and realised by writing record r floor(w_r) or ceil(w_r) times.  The 265-byte record,
 * the search, the moves, dice, games, pi and z are those of the same run without the feature.
 * All arithmetic below is fp32, each operation rounded on its own (no fused multiply-add), in the order written.
 *
 * ln32(x), the engine's own logarithm:
 *     if (x < 1.17549435e-38f) x = 1.17549435e-38f;                         (zero and subnormals included)
 *     b = the bits of x;   e = (int)(b >> 23) - 127;   m = the float with bits (b & 0x7FFFFF) | 0x3F800000
 *     if (m > 1.41421354f) { m = m * 0.5f;  e += 1; }
 *     t = (m - 1) / (m + 1);   t2 = t * t
 *     p = 0.111111112f;   then p = p * t2 + c for c = 0.142857149f, 0.2f, 0.333333343f, 1.0f in turn (a multiply, then an add)
 *     ln32 = (float)e * 0.693147182f + (2.0f * t) * p
 * Against the double logarithm on (1e-38, 2]: relative error below 5e-7 where |ln x| > 1e-3, absolute error below 1.6e-5;
 * ln32(1) = 0 exactly.
 *
 * Surprise of a record, computed when it is staged.  pi = the policy that goes into the record (the pruned one under policy target
 * pruning); P = the root node's stored prior row, before any noise (what azr_mcts_root_stats reports); valid = the root's legal moves.
 *     term[m] = pi[m] * (ln32(pi[m]) - ln32(P[m]))   for a legal m with pi[m] > 0,  else 0
 *     KL = term[0] + term[1] + ... + term[42] summed one after the other from 0.0f in index order;   KL = max(KL, 0)
 *
 * Weights of a finished game with n staged records KL_0 .. KL_{n-1} in staging order:
 *     S = KL_0 + ... + KL_{n-1} summed one after the other from 0.0f
 *     !(S > 0):   w_r = 1 for every r
 *     else        w_r = (1.0f - share) + (share * (float)n) * (KL_r / S);   w_r = min(w_r, max_weight)
 *
 * Copies.  r = the record's ordinal among the game's staged records: 0 for the first record staged since the game — or an entry
 * through azr_selfplay_start*_from_states — began; under a playout cap only full decisions are staged, so r counts those.
 * s = the game's seed; mix as in the playout cap's coin:
 *     base = (uint32)w_r (truncated);   fr = w_r - (float)base;   thr = (uint32)(fr * 16777216.0f)
 *     k = mix(seed + 0x165667B1);   k = mix(k ^ s);   k = mix((k ^ r) + 0xD3A2646C)
 *     c_r = base + ((k >> 8) < thr)
 * The two constants are neither the Dirichlet sampler's (0x9E3779B9, 0x85EBCA6B) nor the playout cap's (0xC2B2AE35, 0x27D4EB2F), so
 * equal seeds do not tie the copies to the noise or to the kind of a decision.  The copy count is a function of (seed, s, r, the
 * game's pi and P) alone: not of the slot, the number of games or threads, the pass schedule or the other seeds; nothing is drawn
 * from the game's own RNG stream.  An exact integer w_r has thr = 0 and never gets an extra copy.
 *
 * Flush.  A finished game reserves C = sum of c_r ring records in one reservation and writes record r c_r times, copies adjacent, in
 * staging order; a record with c_r = 0 is not written.  Records past the ring's end are dropped and counted in records_dropped as
 * without the feature.  Counters: samples counts C; every other counter is that of the same run without the feature.
 * The arena (azr_arena_*), the host-stepped searches (azr_mcts_*) and scripted collection never see it.
 *
 * share <= 0 = off (default).  Read by azr_selfplay_start*; a running self-play never sees a change.  max_weight is the caller's
 * choice (it is not read while off).  AZR_E_INVALID_ARGUMENT, with a reason in azr_last_error, for a NaN, for share > 1, or — when
 * on — a max_weight outside [1, 64]. */
int azr_selfplay_set_surprise_weighting(azr_engine* h, float share, float max_weight, uint32_t seed);
/* the rule alone, on the device, one wavefront per game through the device functions of the self-play step: pi, prior [rows][43] and
 * valid [rows] hold the games' records one game after the other, rows = the sum of game_len[i], i < games; game_seed[i] = the game's
 * seed s.  kl_out, w_out, copies_out [rows].  share in (0, 1], max_weight in [1, 64]. */
int azr_debug_surprise_weights(azr_engine* h, float share, float max_weight, uint32_t seed, const float* pi, const float* prior,
                               const uint64_t* valid, const uint32_t* game_len, const uint32_t* game_seed, int games,
                               float* kl_out, float* w_out, uint32_t* copies_out);

/* ---- value mix: the search's root value blended into the records' z (this engine's own; off after azr_engine_create) ----
 * The reference writes the bare game outcome z in {-1, 0, +1} into bytes 89..92 of every record of a finished game: the first-round
 * record and the last-move record of a game decided by dice carry the same value.  With the value mix (Lc0's q_ratio; z/q averaging
 * in Oracle's "Lessons from AlphaZero") a record's value target is the average of the outcome and the value the search found at that
 * root.  The 265-byte record format, the search, the moves, dice, games, pi and every counter are those of the same run without the
 * feature; only bytes 89..92 differ.
 * All arithmetic below is fp32, each operation rounded on its own (no fused multiply-add), in the order written.
 *
 * Root value of a finished search.  N[m], Q[m] = the root node's completed visits and mean values as the search left them (what
 * azr_mcts_root_stats reports; N is the unpruned count, the low 24 bits of the node's N word); valid = the root's legal moves.
 *     num = 0.0f;  den = 0.0f
 *     for m = 0 .. 42 in index order, if m is legal and N[m] > 0:
 *         num = num + (float)N[m] * Q[m]                                     (a multiply, then an add)
 *         den = den + (float)N[m]
 *     has_q = den > 0
 *     q = num / den;   q = min(max(q, -1.0f), 1.0f)                           (only where has_q; q = 0 without it)
 * Q[m] is from the root mover's perspective (the backup flips the sign once per change of player below the entry), so q has the
 * perspective of the record's z: that of the record's player, byte 0.
 *
 * Blend, when the finished game's records are written.  z = the outcome for the record's player, as without the feature.
 *     a  = 1.0f - q_share
 *     z' = has_q ? a * z + q_share * q : z                                    (two multiplies, then an add)
 *     z' = min(max(z', -1.0f), 1.0f)
 * z' goes into bytes 89..92; nothing else in the record changes.  q_share = 1 gives z' = q exactly; a drawn game gives q_share * q.
 *
 * With the other self-play settings.  Playout cap: a fast decision stages no record, so it has nothing to blend.  Policy target pruning
 * changes pi only: q comes from the unpruned N and Q, the search that chose the move.  Surprise weighting: every copy of a record
 * carries the same z'; KL, weights, copy counts and `samples` are unchanged.  The arena (azr_arena_*, collected samples included),
 * scripted collection and the host-stepped searches (azr_mcts_*) never see it.
 *
 * q_share <= 0 = off (default).  Read by azr_selfplay_start*; a running self-play never sees a change.  AZR_E_INVALID_ARGUMENT, with a
 * reason in azr_last_error, for a NaN or q_share > 1. */
int azr_selfplay_set_value_mix(azr_engine* h, float q_share);
/* q of the last search's roots, q_host [G], computed on the device by the device function the self-play step uses; has_q_host [G]
 * (optional) 1 where the root has a completed visit.  A root that is not in the tree reports 0 with has_q 0.  Valid wherever
 * azr_mcts_root_stats is. */
int azr_mcts_root_value(azr_engine* h, float* q_host /*[G]*/, uint8_t* has_q_host /*[G], optional*/);
/* the rule alone, on the device, one wavefront per row through the device functions of the self-play step and its flushes: N, Q
 * [rows][43], valid, z [rows] -> q_out, has_q_out, z_out [rows].  q_share in (0, 1]. */
int azr_debug_value_mix(azr_engine* h, float q_share, const uint32_t* N, const float* Q /*[rows][43]*/, const uint64_t* valid,
                        const float* z /*[rows]*/, int rows, float* q_out, uint8_t* has_q_out, float* z_out);

/* ---- resignation with a no-resign holdout (this engine's own; off after azr_engine_create) ---------------------------
 * The reference plays every self-play game to its last dice roll: a game that is decided long before it ends still pays
 * mcts_simulations at each of its closing decisions.  With resignation (AlphaGo Zero, KataGo) a player whose root value stays below a
 * bound for `streak` of its own recorded decisions in a row gives the game up.  A share of the games is held out: such a game never
 * resigns, plays on, and reports at its natural end how often the player who would have resigned did not lose — the rule's false
 * positives.  The search never depends on it: up to the decision at which it ends, a resigning game is the game without the feature,
 * record for record but for z.
 * All arithmetic is fp32.  q and has_q are those of the value mix (see "Root value of a finished search" above), from the root's
 * unpruned N and its Q when the decision's search has finished.  p = the mover at the root, byte 0 of the record.
 *
 * Per-game state, zeroed when a game starts or is entered through azr_selfplay_start*_from_states: run[0], run[1], 8-bit counters that
 * saturate at 255; first, one of {none, 0, 1}.
 *
 * Holdout coin of a game with seed s; mix as in the playout cap's coin:
 *     k = mix(seed + 0x2545F491);   k = mix(k ^ s);   k = mix(k + 0x68E31DA4)
 *     holdout  <=>  (k >> 8) < (uint32_t)(holdout_share * 16777216.0f)        (the threshold is computed once, on the host, in float)
 * The coin is a function of (seed, s, holdout_share) alone: not of the slot, the number of games or threads or the pass schedule; it
 * is recomputed from the game's seed and never stored, and nothing is drawn from the game's own RNG stream.  The two constants are
 * none of the Dirichlet sampler's (0x9E3779B9, 0x85EBCA6B), the playout cap's (0xC2B2AE35, 0x27D4EB2F) or the copy coin's
 * (0x165667B1, 0xD3A2646C).  holdout_share = 1 holds every game out, 0 none.
 *
 * At a decision — under a playout cap at a full decision only; a fast decision neither reads nor changes the state — after the
 * decision's record (with its surprise and root value, if in force) has been staged as without the feature, and before the pick:
 *     below  = has_q && q < q_resign
 *     run[p] = below ? min(run[p] + 1, 255) : 0                               (the other player's run is untouched)
 *     gives_up = run[p] >= streak
 * gives_up in a game that is not held out: the game ends here — no pick, no rFloat, no move.  Its status is 1 - p, a win for the
 * opponent; its staged records, the resigning decision's included, are flushed with that status through the flush of any finished game
 * (so the value mix, surprise copies and `samples` work as for any finished game); `decisions` counts the resigning decision,
 * `games_finished` the game (a quota run still ends at games_finished + errors == games); the slot takes its next game exactly as
 * after a natural end.
 * gives_up in a held-out game: nothing in play changes; if first is none, first = p.
 * When a held-out game ends naturally with status st: holdout_games += 1; if first is not none, holdout_would_resign += 1, and if
 * st != 1 - first (the would-be resigner won or drew) holdout_not_lost += 1.  A game abandoned on a rules error counts nowhere.
 *
 * Whether and where a game resigns is a function of its seed, its searches and the four arguments alone.  The arena (azr_arena_*),
 * scripted collection and the host-stepped searches (azr_mcts_*) never see it.
 *
 * streak <= 0 = off (default).  q_resign is a plain bound on q (a typical value is -0.9; it may be positive).  Read by
 * azr_selfplay_start*; a running self-play never sees a change.  AZR_E_INVALID_ARGUMENT, with a reason in azr_last_error, for a NaN,
 * or — when on — q_resign outside [-1, 1], streak > 255 or holdout_share outside [0, 1]. */
int azr_selfplay_set_resign(azr_engine* h, float q_resign, int streak, float holdout_share, uint32_t seed);
typedef struct azr_resign_stats {
    uint64_t resigned;              /* games that ended by resignation (they count in games_finished too) */
    uint64_t holdout_games;         /* held-out games that ended naturally */
    uint64_t holdout_would_resign;  /* ... of them, those in which a player reached the streak */
    uint64_t holdout_not_lost;      /* ... of those, the ones the first such player won or drew: the false positives */
} azr_resign_stats;
/* Kept per game slot by the slot's own wavefront, without atomics, and summed here; reset wherever azr_selfplay_counters' are. */
int azr_selfplay_resign_stats(azr_engine* h, azr_resign_stats* out);
/* the state of each slot's running game: run_host [G][2], first_host [G] (255 = none), holdout_host [G] (the coin of the game's seed;
 * 0 for a slot that has gone idle).  All 0 / 255 / 0 when resignation is off or the engine is not in self-play. */
int azr_selfplay_resign_state(azr_engine* h, uint8_t* run_host /*[G][2]*/, uint8_t* first_host /*[G]*/, uint8_t* holdout_host /*[G]*/);
/* the rule alone, on the device, one wavefront per game through the device functions of the self-play step: q, has_q, player [rows]
 * hold the games' decisions one game after the other, rows = the sum of game_len[i], i < games; game_seed[i] = the game's seed s.
 * resign_row_out [games] = the row within the game at which the streak is first reached, or -1; resigner_out [games] = that row's
 * player, or 255 — both for held-out games too; holdout_out [games] = the coin.  streak in [1, 255]. */
int azr_debug_resign(azr_engine* h, float q_resign, int streak, float holdout_share, uint32_t seed, const float* q, const uint8_t* has_q,
                     const uint8_t* player /*[rows]*/, const uint32_t* game_len, const uint32_t* game_seed, int games,
                     int32_t* resign_row_out, uint8_t* resigner_out, uint8_t* holdout_out /*[games]*/);

/* ---- Gumbel root search with sequential halving (this engine's own; off after azr_engine_create) ---------------------
 * The reference selects by PUCT at every level and records the root's visit distribution; at 16 to 100 simulations over up to 43 moves
 * that target is a coarse copy of the prior, and nothing makes it an improvement on the prior.  Gumbel AlphaZero (Danihelka, Guez,
 * Schrittwieser, Silver, "Policy improvement by planning with Gumbel", ICLR 2022) samples the root's candidate moves without
 * replacement through Gumbel noise, spends the budget on them by sequential halving, plays the winner and records
 * softmax(logit + sigma(completed Q)).  Here it replaces the selection at path depth 0 and the decision; deeper levels keep PUCT
 * unless "selection below the root" (further down) is switched on, and the arena (azr_arena_*) never sees it.
 * All arithmetic below is fp32, each operation rounded on its own (no fused multiply-add), in the order written; lane i <-> move i.
 *
 * Per root.  P = the node's stored prior row (azr_mcts_root_stats);  logit[a] = ln32(max(P[a], 1.17549435e-38f)) with the ln32 of
 * "policy surprise weighting";  valid = the node's legal moves;  n = the search budget in force, S - S % T;  m_eff = min(m, the number
 * of legal moves);  N, Q = the node's rows, act[a] = the visits of a in flight in other search threads (the top byte of the N word).
 * N0 = the root's N row at the moment this search made its first root-level selection (kept per game; a root that tree reuse brought
 * along starts with N0 = N);  ns[a] = N[a] > N0[a] ? N[a] - N0[a] : 0, the search-local count of completed visits.
 *
 * exp32(x), the engine's own exponential for x <= 0:
 *     if (x < -104.0f) return 0
 *     kf = rint(x * 1.44269502f) (to nearest, ties to even);   k = (int)kf
 *     r = (x - kf * 0.693145752f) - kf * 1.42860682e-06f
 *     p = 1.98412701e-04f;   then p = p * r + c for c = 1.38888892e-03f, 8.33333377e-03f, 4.16666679e-02f, 1.66666672e-01f, 0.5f,
 *         1.0f, 1.0f in turn (a multiply, then an add)
 *     k1 = k >> 1 (arithmetic);   exp32 = (p * 2^k1) * 2^(k - k1)                (the two powers of two are exact floats)
 * Against the double exponential on a grid of [-104, 0] (tests/test_gumbel_ref.py): relative error at most 9.84e-8 where the result is
 * a normal float, at most 0.775 of the smallest denormal below that; exp32(0) = 1 exactly; no argument <= 0 gives a NaN.
 *
 * The Gumbel vector of a root.  d = the decisions already taken in the running game, s = the game's seed, as in the playout cap's coin,
 * whose mix this is:
 *     k = mix(seed + 0xB5297A4D);   k = mix(k ^ s);   k = mix((k ^ d) + 0x1B56C4E9);   k_a = mix(k ^ ((a + 1) * 0x9E3779B9))
 *     u = ((float)(mix(k_a) >> 9) + 0.5f) * 2^-23                                   (the first uniform of the Dirichlet sampler's stream k_a)
 *     g[a] = -ln32(-ln32(u))   for a legal a,   0 for an illegal one
 * The two constants are nobody else's (Dirichlet 0x9E3779B9, 0x85EBCA6B; cap 0xC2B2AE35, 0x27D4EB2F; copies 0x165667B1, 0xD3A2646C;
 * holdout 0x2545F491, 0x68E31DA4).  g is a function of (seed, s, d, a) alone; nothing is drawn from the game's own RNG stream.  A root
 * whose round is above temperature_threshold gets g = 0 everywhere: the greedy late game, so the threshold keeps its meaning.
 *
 * Net value of a node, vhat: the value the net returned when the node was expanded, for the node's mover (the sign the backup takes).
 * It is kept in the node — the float behind its 43 priors, which is 0 in every node a search without the feature expands — so it
 * survives tree reuse; switching the feature on clears the trees, so no node without a vhat is searched.
 *
 * Completed Q.
 *     seen[a] = a is legal and N[a] > 0;   total = the integer sum of N over the legal moves
 *     wp = the sum of P[a], wq = the sum of P[a] * Q[a] over the seen moves, each summed one after the other from 0.0f in index order
 *     v_mix = (total > 0 && wp > 0) ? (vhat + (float)total * (wq / wp)) / (1.0f + (float)total) : vhat
 *     qhat[a] = seen[a] ? Q[a] : v_mix
 *     sigma[a] = ((c_visit + (float)(the largest N of a legal move)) * c_scale) * qhat[a]
 * Values lie in [-1, 1] and are not rescaled.  The paper rescales them to [0, 1], q01 = (q + 1) / 2, so the paper's [0, 1] convention
 * is half this c_scale's effect per unit: its c_scale of 1.0 is 0.5 here.
 *
 * Considered visits, cv(m_eff, n, i) for the claim index i = 0 .. n - 1 (the i-th descent the search starts):
 *     m_eff <= 1:  cv = i.
 *     else L = ceil(log2 m_eff), k = m_eff, base = 0, and until n entries exist:  e = max(1, n / (L * k)) (integer);  for j = 0 .. e - 1
 *     emit k entries equal to base + j;  base += e;  k = max(2, k / 2).
 * m_eff = 4, n = 16 gives 0,0,0,0,1,1,1,1,2,2,3,3,4,4,5,5 and the search-local visits (6, 6, 2, 2).  It is recomputed from i, never stored.
 *
 * Root-level selection of claim i (path depth 0 only):
 *     cnt[a] = ns[a] + act[a]
 *     candidates = the legal moves with cnt == cv;  if there is none, the legal moves with the largest cnt below cv;  if there is still
 *     none (a root that a transposition visited from below), all legal moves
 *     the move = the candidate with the largest (g + logit) + sigma, the lowest index on ties
 * with the bookkeeping of the PUCT selection (the in-flight count of the move goes up, the node counts as visited).  The first m_eff
 * claims all see qhat = v_mix on the unvisited moves and so take the m_eff best by g + logit: the sample without replacement.
 *
 * Decision.  The move = the legal move with the largest ns, among those the largest (g + logit) + sigma, the lowest index on ties;
 * nothing is drawn, so a Gumbel decision takes no rFloat from the game's stream.  The record's pi:
 *     x[a] = logit[a] + sigma[a] on the legal moves;  mx = their maximum;  e[a] = exp32(x[a] - mx);  sum = e[0] + .. + e[42] one after the
 *     other from 0.0f with 0 for an illegal move;  pi[a] = e[a] / sum, 0 for an illegal move.
 * Staging, z back-fill, game turnover, quota, surprise weighting (on this pi), the value mix and resignation (on the node's N and Q)
 * work as without the feature.
 *
 * Selection below the root (the paper's deterministic non-root selection, its "Full Gumbel" search; off by default).  On, it takes the
 * PUCT selection's place at every node met at path depth >= 1 of a descent — the root's own state included, when a transposition
 * reaches it from below; path depth 0 keeps the root-level selection above.  The node spends its visits in proportion to its own
 * improved policy.  N, act, Q, P, vhat, valid = this node's rows:
 *     pi'[a]   = the record's pi above, computed on this node's rows (logit, the completed Q with the node's own vhat, sigma with the
 *                node's largest N, exp32, the 43-term sums in index order); 0 on an illegal move
 *     cnt[a]   = N[a] + act[a];   tot = the integer sum of cnt over the legal moves
 *     den      = 1.0f + (float)tot
 *     score[a] = pi'[a] - (float)cnt[a] / den                                    (a divide, then a subtract)
 *     the move = the legal move with the largest score, the lowest index on ties
 * with the bookkeeping of the PUCT selection (the in-flight count of the move goes up, the node counts as visited).  No N0 is
 * involved: below the root the node's all-time counts are the paper's N.  Nothing is drawn, no rFloat is taken, and c_visit and
 * c_scale are the root's.  Applied n times from empty counts under a fixed pi', the rule keeps |N[a] - n pi'[a]| below 1
 * (tests/test_gumbel_tree_ref.py).
 *
 * Device self-play: m = 0 = off (default); read by azr_selfplay_start*, a running self-play never sees a change.
 * AZR_E_INVALID_ARGUMENT, with a reason in azr_last_error, for m outside [0, 43], a c_visit or c_scale that is not finite, or — when
 * on — c_visit < 0 or c_scale <= 0.  azr_selfplay_start* returns AZR_E_INVALID_ARGUMENT, with a reason, when the Gumbel search is set
 * together with Dirichlet noise, a playout cap or forced playouts; the handle stays as it was. */
int azr_selfplay_set_gumbel(azr_engine* h, int m, float c_visit, float c_scale, uint32_t seed);
/* the selection below the root of a device self-play: on = 0 (default) = PUCT, 1 = the rule above.  Read by azr_selfplay_start*, a
 * running self-play never sees a change.  AZR_E_INVALID_ARGUMENT for any other value; azr_selfplay_start* returns
 * AZR_E_INVALID_ARGUMENT, with a reason, when it is 1 while azr_selfplay_set_gumbel's m is 0, and the handle stays as it was. */
int azr_selfplay_set_gumbel_tree(azr_engine* h, int on);
/* host-stepped searches (azr_mcts_simulate / azr_mcts_begin..apply): the same search under the vector of azr_mcts_set_root_gumbel.
 * Holds until set again; azr_selfplay_start* ends it.  Switching it on or off clears the trees, and so does the first azr_mcts_begin /
 * azr_mcts_simulate after an arena while it is on (the arena's searches expand nodes without a vhat).  Refused
 * (AZR_E_INVALID_ARGUMENT) while a root noise vector or forced playouts are in force, as those two setters are while it is. */
int azr_mcts_set_gumbel(azr_engine* h, int m, float c_visit, float c_scale);
/* ... and its selection below the root: on = 0 or 1.  Refused (AZR_E_INVALID_ARGUMENT) while no host-stepped Gumbel search is in force;
 * azr_mcts_set_gumbel(h, 0, ...) puts it back to 0.  Toggling it does not clear the trees: every node a Gumbel search expanded has its
 * vhat either way. */
int azr_mcts_set_gumbel_tree(azr_engine* h, int on);
/* g_host [G][43]: the vector of each game's root for the searches that follow, used as given; NULL = zeros */
int azr_mcts_set_root_gumbel(azr_engine* h, const float* g_host);
/* the vector in force at each game's current root, g_host [G][43] (a running self-play's draws, or what was set); zeros when no
 * Gumbel search is in force */
int azr_mcts_root_gumbel(azr_engine* h, float* g_host);
/* of the last search's roots, by the device functions of the self-play decision: the record's pi, pi_host [G][43], and (optional)
 * the completed Q, qhat_host [G][43], 0 on illegal moves; the decision's move, moves_host [G] (43 for a root that is not in the
 * tree).  AZR_E_STATE when no Gumbel search is in force. */
int azr_mcts_gumbel_policy(azr_engine* h, float* pi_host, float* qhat_host /*optional*/);
int azr_mcts_gumbel_pick(azr_engine* h, uint8_t* moves_host);
/* the draw alone, on the device: g_out [rows][43] for (game_seed[i], decision[i], valid[i], greedy[i] != 0 = a root above the threshold) */
int azr_debug_root_gumbel(azr_engine* h, uint32_t seed, const uint32_t* game_seed, const uint32_t* decision, const uint64_t* valid,
                          const uint8_t* greedy, int rows, float* g_out);
/* the root-level selection alone, on the device, one wavefront per synthetic row: N, N0, act, Q, P, g [rows][43], vhat, valid and the
 * claim index [rows] -> the move (43 = none) and cv.  m in [1, 43], n > 0. */
int azr_debug_gumbel_select(azr_engine* h, int m, int n, float c_visit, float c_scale, const uint32_t* N, const uint32_t* N0,
                            const uint32_t* act, const float* Q, const float* P, const float* g, const float* vhat,
                            const uint64_t* valid, const uint32_t* claim, int rows, uint8_t* move_out, uint32_t* cv_out);
/* the selection below the root alone, on the device, one wavefront per synthetic row: N, act, Q, P [rows][43], vhat, valid [rows] ->
 * the move (43 = none) and score [rows][43], 0 on an illegal move.  c_visit >= 0, c_scale > 0. */
int azr_debug_gumbel_tree_select(azr_engine* h, float c_visit, float c_scale, const uint32_t* N, const uint32_t* act, const float* Q,
                                 const float* P /*[rows][43]*/, const float* vhat, const uint64_t* valid /*[rows]*/, int rows,
                                 uint8_t* move_out /*[rows]*/, float* score_out /*[rows][43]*/);
/* exp32 alone, on the device: out[i] = exp32(x[i]), i < n */
int azr_debug_exp32(azr_engine* h, const float* x, int n, float* out);

/* ---- device-resident self-play (trainer move loop, alphazero_trainer.cpp:80-119) --------------------------- */
/* (Re)start all G games: game g plays seeds base_seed + g, then base_seed + G + g, ... */
int azr_selfplay_start(azr_engine* h, uint32_t base_seed);
/* The trainer's own loop bound (Counter::hasNext over TRAIN_ITERATION_GAMES, alphazero_trainer.cpp:83): start exactly
 * `games` games — seeds base_seed .. base_seed + games - 1, handed to whichever slot is free next — and play every one
 * of them to its end; slots idle once no game is left to start.  Done when games_finished + errors == games. */
int azr_selfplay_start_games(azr_engine* h, uint32_t base_seed, uint64_t games);
/* The move loop entered in the MIDDLE of games: game g goes on from the state and RNG stream the caller has set
 * (azr_engine_set_states / azr_engine_set_rng; states must be running games), its records start there; a finished game's
 * slot restarts as under azr_selfplay_start (seeds base_seed + G + g, base_seed + 2G + g, ...). */
int azr_selfplay_start_from_states(azr_engine* h, uint32_t base_seed);
/* Both at once: the games of slots 0 .. min(games, G) - 1 go on from the states and RNG streams the caller has set, seeds
 * base_seed + slot; the other slots idle.  With games <= G no further game is started: the run is over when those games are. */
int azr_selfplay_start_games_from_states(azr_engine* h, uint32_t base_seed, uint64_t games);
/* Run `passes` passes of the hot path: every pass = one tree step (backup/expand + select to the next leaf,
 * decisions, moves, game restarts — all on device) + one batched net evaluation of the G leaves. */
int azr_selfplay_run(azr_engine* h, int passes);
typedef struct azr_counters {
    uint64_t simulations;   /* completed search() descents (root expansions not counted) */
    uint64_t evaluations;   /* net evaluations consumed (leaf + root) */
    uint64_t levels;        /* inner-node levels visited (mean depth = levels / simulations) */
    uint64_t decisions;     /* moves played */
    uint64_t games_finished;
    uint64_t samples;       /* records produced */
    uint64_t nodes_dropped; /* expansions skipped because the node pool was full, plus the nodes evicted when a root expansion found
                               it full and emptied the tree (should be 0) */
    uint64_t errors;        /* games stopped on a rules error (should be 0) */
    uint64_t records_dropped; /* records lost because a game outgrew sample_capacity or the ring was full (should be 0;
                                 `samples` counts them too) */
    uint64_t tower_fallbacks; /* net launches of <= 128 boards (split-channel tower, 4 co-resident workgroups per board pair) in which a
                                 workgroup waited for its partners longer than the spin limit — the GPU was shared with something that kept
                                 them from running — and which the one-board-per-workgroup kernel queued behind them recomputed, in
                                 stream order: results are unaffected, the count says how often it happened since the handle exists
                                 (normally 0) */
} azr_counters;
int azr_selfplay_counters(azr_engine* h, azr_counters* out);
/* finished games' records, z filled (NNTrainDataStorage::updateValues, alphazero_nn_data.cpp:51-65).  Copies the first
 * min(available, cap_records) records; the others STAY buffered for the next call (drain in a loop until *n_out <
 * cap_records).  rec265_host == NULL discards everything buffered. */
int azr_samples_drain(azr_engine* h, void* rec265_host, size_t cap_records, size_t* n_out);
/* the same copy to DEVICE memory of this GPU (e.g. a collective's send buffer), on the engine's own stream, without
 * removing anything: min(available, cap_records) records */
int azr_samples_copy_device(azr_engine* h, void* rec265_device, size_t cap_records, size_t* n_out);
/* device-side view for RCCL gathers: pointer to the packed record ring and its count; valid until the next
 * azr_selfplay_run / azr_samples_drain */
int azr_samples_device_view(azr_engine* h, void** dev_ptr_out, size_t* n_out);

/* ---- arena: GameGroup::playGames (game/game.cpp:256-312) on the device ------------------------------------------------ */
/* The G slots of the engine are the reference's G player pairs (threads): each plays Game::playGames(1) repeatedly —
 * mirrored pairs with alternating starts (Game::newGame, game.cpp:170-191) — until Counter::hasNext(2) fails.
 * Players: AlphaZeroPlayer (alphazero_player.cpp:3-21, argmax, tree trimmed at every turn), ScriptPlayer
 * (player/script/script_player.cpp), RandomPlayer (player/random/random_player.cpp). */
enum { AZR_PLAYER_ALPHAZERO = 0, AZR_PLAYER_SCRIPT = 1, AZR_PLAYER_RANDOM = 2,
       AZR_PLAYER_ALPHAZERO_B = 3 /* AlphaZeroPlayer on a second network: azr_arena_set_opponent_net */ };
typedef struct azr_game_results {   /* GameResults (game/game.h:17-29) */
    int32_t count, draw;
    int32_t win[2], win_and_started[2];
} azr_game_results;
/* mirror_games (SETTINGS.MIRROR_GAMES, game.cpp:170-191):
 *   AZR_MIRROR_OFF         every game a fresh deal
 *   AZR_MIRROR_SEQUENTIAL  the reference's thread-per-pair form: a slot deals, plays the game, then plays the same deal with the
 *                          players inverted (State::invertPlayers, state.cpp:493-516); slot g draws everything — deals and dice of
 *                          all its games — from ONE minstd_rand0 stream seeded base_seed + g (the reference's global engine)
 *   AZR_MIRROR_CONCURRENT  the two games of a pair at the same time on the slots 2j and 2j + 1 (nothing in Game orders them, only
 *                          the shared initial deal does).  Pair p = j + k (G/2) is the k-th pair of slot pair j; both halves deal from
 *                          minstd_rand0(base_seed + p); half 0 (player 0 starts) goes on with that stream for its dice, half 1
 *                          (invertPlayers of the same deal, player 1 starts) draws its dice from minstd_rand0(base_seed + p + 2^30).
 *                          Pairs are assigned statically (p < games / 2), so a run is a function of its arguments alone; G even.
 * games = Counter::count; games_per_slot_cap > 0 additionally limits every slot (deterministic splits for tests) */
enum { AZR_MIRROR_OFF = 0, AZR_MIRROR_SEQUENTIAL = 1, AZR_MIRROR_CONCURRENT = 2 };
int azr_arena_start(azr_engine* h, int player1, int player2, int games, int games_per_slot_cap, int mirror_games,
                    uint32_t base_seed);
int azr_arena_run(azr_engine* h, int passes, int* finished_out);
/* New-vs-old arena (GameGroup::playGames(trainAZPG, generateAZPG, ...), alphazero_trainer.cpp:147-152): player
 * AZR_PLAYER_ALPHAZERO_B searches a tree of its own in every slot (every AlphaZeroPlayer owns an AlphaZeroMCTS) and is
 * evaluated by `other`'s network (same device, at least h's leaf slots; its blocks and net_dtype may differ from h's;
 * `other` may be h itself; its weights are used in place, so keep `other` alive and pass NULL here before destroying
 * it).  Each pass runs the two networks on the leaves of their own players only. */
int azr_arena_set_opponent_net(azr_engine* h, azr_engine* other);
/* Search settings of player AZR_PLAYER_ALPHAZERO_B in this handle's arena: its simulations per decision and its PUCT
 * constant (every AlphaZeroPlayer's AlphaZeroMCTS reads its own Settings).  mcts_simulations < 0 / hp_exploration < 0 = this
 * handle's own (the state after azr_engine_create and after azr_arena_set_opponent_net(h, NULL)).  mcts_threads stays the
 * handle's (leaf slot = g * T + k for both trees), so mcts_simulations >= mcts_threads and the count per decision is
 * S - S % T.  Player B's tree lives in this handle's second node pool, which has the first one's size: a budget whose default
 * pool 16 * (mcts_simulations + 1) exceeds it is AZR_E_INVALID_ARGUMENT (create the handle with a larger node_capacity).
 * AZR_E_STATE between azr_arena_start and the arena's finish, i.e. the azr_arena_run that reports *finished_out = 1 (starting
 * self-play or a host-stepped search ends an arena too).  azr_arena_start reads the setting: a running arena never sees a change,
 * the reset through azr_arena_set_opponent_net(h, NULL) included.  The setting holds over later azr_arena_start calls until it is
 * set again.  Player AZR_PLAYER_ALPHAZERO, self-play, the one-net arenas and azr_mcts_* keep the handle's settings. */
int azr_arena_set_opponent_search(azr_engine* h, int mcts_simulations, float hp_exploration);
/* The Gumbel search of azr_selfplay_set_gumbel (every definition is the one stated there) for one AlphaZero player of this handle's
 * arenas: player = AZR_PLAYER_ALPHAZERO or AZR_PLAYER_ALPHAZERO_B.  m = 0 (default) = off, the side searches by PUCT and plays bit for
 * bit what it plays without this call, whatever the other side does.  A side with m > 0 plays every one of its decisions like this:
 *   root vector   g = 0 on every move, as at a self-play root above temperature_threshold: nothing is drawn, there is no seed, and
 *                 the arena stays a function of its arguments.
 *   search        the root-level selection for the claim index i = the descents this search has started before.  n = this side's
 *                 simulations per decision (S - S % T; player B's of azr_arena_set_opponent_search), m_eff = min(m, legal moves), N0 =
 *                 the root's N row at this search's first root-level selection — the arena keeps a player's tree inside a turn, so
 *                 N0 is non-zero from a turn's second decision on.  Below the root: PUCT with the side's own hp (tree = 0), or the
 *                 selection below the root stated above (tree = 1), under this side's c_visit and c_scale.
 *   vhat          in an arena with a Gumbel side every expansion stores the net's value in the node, in both players' trees; both
 *                 trees are emptied at every deal, so no node without a vhat is ever searched.
 *   decision      the move = the Decision above with g = 0; with azr_arena_collect_samples on, the record's pi is the record's pi
 *                 above (what a self-play Gumbel record carries) in place of the visit distribution.  z, the flush order and every
 *                 counter are what they are without the feature.
 * From the same state, RNG word and tree contents a decision gives the root's N and Q, the move and the pi of a host-stepped search
 * under azr_mcts_set_gumbel(m, c_visit, c_scale), azr_mcts_set_gumbel_tree(tree), azr_mcts_set_root_gumbel(NULL),
 * azr_mcts_set_simulations(n) and the side's hp (tests/arena_retrace.py).
 * AZR_E_INVALID_ARGUMENT, with a reason in azr_last_error, for another player, m outside [0, 43], a c_visit or c_scale that is not
 * finite, with m > 0 a c_visit < 0 or c_scale <= 0, a tree other than 0 or 1, and tree = 1 with m = 0.  Lifetime as
 * azr_arena_set_opponent_search's: read by azr_arena_start; AZR_E_STATE between azr_arena_start and the arena's finish; holds over later
 * arenas until set again; player B's goes back to off with azr_arena_set_opponent_net(h, NULL).  A setting for a player that an arena
 * does not have leaves that arena as it is.  azr_arena_start returns AZR_E_INVALID_ARGUMENT, with a reason and the handle unchanged,
 * when a side of the arena has m > 0 while azr_arena_collect_scripted_samples is on.  Independent of azr_selfplay_set_gumbel and
 * azr_mcts_set_gumbel, which keep their meaning; the first host-stepped Gumbel search after an arena still clears the trees. */
int azr_arena_set_gumbel(azr_engine* h, int player, int m, float c_visit, float c_scale, int tree);
/* INCLUDE_COMPARE_GAMES_TRAIN_SAMPLES (alphazero_trainer.cpp:143-146): AlphaZero players push (s, pi) at every decision
 * (alphazero_player.cpp:15-18); a finished game's records get their z and go to the record ring (azr_samples_drain),
 * game by game in decision order (the reference appends player by player).  Set before azr_arena_start.  Its sibling
 * azr_arena_collect_scripted_samples records the ScriptPlayer / RandomPlayer side; either, both or neither may be on. */
int azr_arena_collect_samples(azr_engine* h, int on);
/* Player::addTrainingSample with a trainStorage attached (player/base/player.cpp:9-17; train-data / train-script,
 * alphazero_trainer.cpp:200-317): ScriptPlayer and RandomPlayer push (player = current player, NNInputData(state),
 * pi = one-hot: 1.0 at the move's index, 0.0 elsewhere, SKIP = 42) with the state as it is at the reference's call sites:
 *   ScriptPlayer (script_player.cpp): setup landAttackFrom :176; setup neutral land :198; every reinforcement step
 *     reinforcmentTo :105; every attack roll landAttackTo :115; every post-capture mobilisation step landAttackTo :125;
 *     fortify landFortifyTo :151, or SKIP :157 when it has lands with army but no fortify move
 *   RandomPlayer (random_player.cpp): setup :29; neutral :35; reinforcement :43; attack target or SKIP :49 (the
 *     attack-from pick is not recorded); mobilisation mobilizationTo on a move :68, mobilizationFrom on a stop :73;
 *     fortify target or SKIP :82
 * Recording draws nothing from the RNG and changes no move.  A finished game's records get z = updateValues
 * (alphazero_nn_data.cpp:51-65) and go to the record ring as one block, in move order: with azr_arena_collect_samples
 * also on, the AlphaZero and scripted records of a game interleave in the order the moves were made (train-data's one
 * shared storage, alphazero_trainer.cpp:240-275).  More than sample_capacity records of one game: the rest are counted
 * in records_dropped.
 * Ring room: a game is dealt only once sample_capacity ring records are reserved for it (given back at its end, less
 * what it wrote).  A slot without room waits, taking nothing from the quota and keeping its seed and pairs, so
 * azr_arena_run may return *finished = 0 only because slots wait for a drain: call azr_samples_drain (all records)
 * after every azr_arena_run, then azr_arena_run again.  Nothing is dropped for want of ring room.
 * Set before azr_arena_start. */
int azr_arena_collect_scripted_samples(azr_engine* h, int on);
int azr_arena_results(azr_engine* h, azr_game_results* out);
/* per slot: games finished, and for its first 16 games status / round count / final state image */
int azr_arena_log(azr_engine* h, int32_t* games_per_slot_host, int8_t* status_host /*[G][16]*/,
                  uint16_t* rounds_host /*[G][16]*/, void* finals160_host /*[G][16][160]*/);

/* ---- measurement hooks (bench.py) --------------------------------------------------------------------------- */
/* average duration in ms of the net-forward launches and of the tree-step launches over the last
 * azr_selfplay_run, measured with HIP events on the engine's stream */
int azr_profile_last_run(azr_engine* h, float* net_ms_avg, float* tree_ms_avg, int* launches);
int azr_device_synchronize(azr_engine* h);
/* diagnostics of the tower kernels (tools/tower_clock.py, tools/tower_trace.py): sustained in-kernel shader clock and
 * workgroup-0 time after `warm` back-to-back launches on n leaf slots; per-workgroup time stamps of one launch */
int azr_debug_tower_clock(azr_engine* h, int n, int warm, double* ghz_out, double* tower_ms_out);
int azr_debug_tower_trace(azr_engine* h, int n, int warm, unsigned long long* out8, int cap_wgs, int* wgs_out);
/* the tile plan of a bf16 net launch of n boards: boards per workgroup (the largest, in a mixed launch) and workgroups;
 * 2..4 boards = k_tower_sb<NB> (one LDS image), 1 = k_tower_bf16<1> (AZR_TOWER_SB=0: k_tower_bf16<1..3>) */
int azr_debug_tower_plan(azr_engine* h, int n, int* boards_per_wg, int* wgs);

#ifdef __cplusplus
}
#endif
#endif /* AZR_H */
