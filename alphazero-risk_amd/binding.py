"""ctypes binding of include/azr.h (libazr_hip.so).  No compute happens in Python."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
NET_F32, NET_BF16, NET_F32X, NET_F16 = 0, 1, 2, 3
MOVES, STATE_BYTES, INPUT_BYTES, RECORD_BYTES = 43, 160, 88, 265


class AzrError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"azr error {code}: {msg}")
        self.code = code


class Settings(C.Structure):
    """`azr_settings` — mirrors the reference's `class Settings` fields the hot path reads (src/settings.h:41-64)."""
    _fields_ = [("device", C.c_int32), ("games", C.c_int32), ("blocks", C.c_int32), ("net_dtype", C.c_int32),
                ("mcts_simulations", C.c_int32), ("mcts_threads", C.c_int32), ("allow_yield", C.c_int32), ("limit_reinforcement", C.c_int32),
                ("limit_attack", C.c_int32), ("max_game_rounds", C.c_int32), ("min_unit_move", C.c_int32),
                ("temperature_threshold", C.c_int32), ("hp_exploration", C.c_float), ("dir_noise_value", C.c_float),
                ("dir_noise_epsi", C.c_float), ("node_capacity", C.c_int32), ("sample_capacity", C.c_int32)]


class GameResults(C.Structure):
    """`azr_game_results` = GameResults (game/game.h:17-29)"""
    _fields_ = [("count", C.c_int32), ("draw", C.c_int32), ("win", C.c_int32 * 2), ("win_and_started", C.c_int32 * 2)]

    def as_dict(self):
        return dict(count=self.count, draw=self.draw, win=list(self.win), win_and_started=list(self.win_and_started))


PLAYER_ALPHAZERO, PLAYER_SCRIPT, PLAYER_RANDOM, PLAYER_ALPHAZERO_B = 0, 1, 2, 3
MIRROR_OFF, MIRROR_SEQUENTIAL, MIRROR_CONCURRENT = 0, 1, 2   # azr_arena_start's mirror_games (include/azr.h)


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("simulations", "evaluations", "levels", "decisions", "games_finished",
                                          "samples", "nodes_dropped", "errors", "records_dropped", "tower_fallbacks")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class ResignStats(C.Structure):   # azr_resign_stats
    _fields_ = [(n, C.c_uint64) for n in ("resigned", "holdout_games", "holdout_would_resign", "holdout_not_lost")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


LR_CONSTANT, LR_COSINE, LR_STEP = 0, 1, 2   # azr_train_options.lr_schedule (include/azr.h)
LR_SCHEDULES = {"constant": LR_CONSTANT, "cosine": LR_COSINE, "step": LR_STEP}


class TrainOptions(C.Structure):   # azr_train_options
    _fields_ = [("lr", C.c_float), ("l2", C.c_float), ("lr_schedule", C.c_int32), ("warmup_steps", C.c_int32), ("total_steps", C.c_int32),
                ("decay_period", C.c_int32), ("decay_gamma", C.c_float), ("lr_min", C.c_float), ("clip_norm", C.c_float), ("ema_decay", C.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class TrainStats(C.Structure):   # azr_train_stats
    _fields_ = [("step", C.c_int64), ("lr", C.c_float), ("lr_t", C.c_float), ("grad_norm", C.c_float), ("clip_scale", C.c_float),
                ("clipped_steps", C.c_int64), ("ema_steps", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int)   # azr_allreduce_fn


def dp_unique_id():
    """azr_dp_unique_id: the 128-byte id rank 0 draws and hands to the other ranks"""
    b = (C.c_uint8 * 128)()
    rc = load_library().azr_dp_unique_id(b)
    if rc:
        raise AzrError(rc, "azr_dp_unique_id: RCCL is not available")
    return bytes(b)


def lib_path(test_hooks=False):
    """the product library, or (test_hooks) libazr_hip_test.so: the same sources compiled with -DAZR_TEST_HOOKS — the only build
    in which the AZR_TOWER_* / AZR_TRAIN_* / AZR_DP_LOOPBACK environment switches exist (csrc/azr_internal.hpp)"""
    return os.path.join(CSRC, "libazr_hip_test.so" if test_hooks else "libazr_hip.so")


def build(jobs=4, test_hooks=False):
    """Compile every HIP translation unit for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-s", "-j", str(jobs), "-C", CSRC, "test" if test_hooks else "all"])
    return lib_path(test_hooks)


_lib = None
_libs = {}

EXPORTS = [
    "azr_default_settings", "azr_engine_create", "azr_engine_destroy", "azr_last_error", "azr_engine_games",
    "azr_engine_new_games", "azr_engine_set_states", "azr_engine_get_states", "azr_engine_set_rng", "azr_engine_get_rng",
    "azr_engine_valid_moves", "azr_engine_make_moves", "azr_engine_status", "azr_engine_encode",
    "azr_nn_param_count", "azr_nn_init_random", "azr_nn_set_weights", "azr_nn_get_weights", "azr_nn_load", "azr_nn_save",
    "azr_nn_predict", "azr_nn_train", "azr_nn_validate", "azr_nn_train_dp", "azr_dp_unique_id", "azr_dp_init", "azr_dp_shutdown", "azr_nn_train_batch", "azr_nn_train_grads", "azr_nn_train_reset", "azr_mcts_clear", "azr_mcts_trim", "azr_mcts_simulate", "azr_mcts_begin", "azr_mcts_leaves",
    "azr_mcts_apply", "azr_mcts_root_stats", "azr_mcts_policy", "azr_mcts_pick", "azr_selfplay_start", "azr_selfplay_start_games", "azr_selfplay_start_from_states",
    "azr_selfplay_run", "azr_selfplay_counters", "azr_samples_drain", "azr_samples_device_view", "azr_samples_copy_device", "azr_profile_last_run",
    "azr_device_synchronize", "azr_debug_tower_clock", "azr_debug_tower_trace", "azr_debug_tower_plan", "azr_arena_start", "azr_arena_run", "azr_arena_results", "azr_arena_log",
    "azr_arena_set_opponent_net", "azr_arena_set_opponent_search", "azr_arena_set_gumbel", "azr_arena_collect_samples", "azr_arena_collect_scripted_samples",
    "azr_mcts_set_root_noise", "azr_selfplay_set_dirichlet", "azr_mcts_root_noise", "azr_debug_root_noise",
    "azr_selfplay_set_playout_cap", "azr_selfplay_decision_kind", "azr_debug_playout_cap",
    "azr_mcts_set_forced_playouts", "azr_mcts_pruned_policy", "azr_selfplay_set_forced_playouts", "azr_mcts_set_simulations",
    "azr_selfplay_start_games_from_states",
    "azr_selfplay_set_surprise_weighting", "azr_debug_surprise_weights",
    "azr_selfplay_set_value_mix", "azr_mcts_root_value", "azr_debug_value_mix",
    "azr_selfplay_set_resign", "azr_selfplay_resign_stats", "azr_selfplay_resign_state", "azr_debug_resign",
    "azr_selfplay_set_gumbel", "azr_mcts_set_gumbel", "azr_mcts_set_root_gumbel", "azr_mcts_root_gumbel", "azr_mcts_gumbel_policy",
    "azr_mcts_gumbel_pick", "azr_debug_root_gumbel", "azr_debug_gumbel_select", "azr_debug_exp32",
    "azr_selfplay_set_gumbel_tree", "azr_mcts_set_gumbel_tree", "azr_debug_gumbel_tree_select", "azr_mcts_node_stats",
    "azr_default_train_options", "azr_nn_train_set_options", "azr_nn_train_get_options", "azr_nn_train_stats", "azr_nn_get_ema_weights",
]


def load_library(test_hooks=False):
    """dlopen libazr_hip.so (or the test-hook build); raises (never falls back) when it has not been built."""
    global _lib
    if test_hooks not in _libs:
        p = lib_path(test_hooks)
        if not os.path.exists(p):
            raise FileNotFoundError(f"{p} missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                    "(the HIP path is the only path; there is no CPU fallback)")
        L = C.CDLL(p)
        L.azr_last_error.restype = C.c_char_p
        L.azr_last_error.argtypes = [C.c_void_p]
        L.azr_nn_param_count.restype = C.c_size_t
        L.azr_nn_param_count.argtypes = [C.c_int]
        L.azr_engine_create.argtypes = [C.c_void_p, C.c_void_p]
        for name in EXPORTS:
            f = getattr(L, name)
            if f.argtypes is None and name not in ("azr_default_settings",):
                pass
        L.azr_nn_init_random.argtypes = [C.c_void_p, C.c_uint64]
        L.azr_nn_set_weights.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.azr_nn_get_weights.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.azr_nn_load.argtypes = [C.c_void_p, C.c_char_p]
        L.azr_nn_save.argtypes = [C.c_void_p, C.c_char_p]
        L.azr_nn_predict.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.azr_nn_train.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.azr_nn_train_dp.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, ALLREDUCE_FN,
                                      C.c_void_p, C.c_void_p, C.c_void_p]
        L.azr_nn_train_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.azr_nn_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.azr_dp_unique_id.argtypes = [C.c_void_p]
        L.azr_dp_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.azr_dp_shutdown.argtypes = [C.c_void_p]
        L.azr_nn_train_grads.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.azr_nn_train_reset.argtypes = [C.c_void_p]
        L.azr_default_train_options.argtypes = [C.c_void_p]
        L.azr_default_train_options.restype = None
        L.azr_nn_train_set_options.argtypes = [C.c_void_p, C.c_void_p]
        L.azr_nn_train_get_options.argtypes = [C.c_void_p, C.c_void_p]
        L.azr_nn_train_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.azr_nn_get_ema_weights.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.azr_selfplay_start.argtypes = [C.c_void_p, C.c_uint32]
        L.azr_selfplay_start_games.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64]
        L.azr_selfplay_start_from_states.argtypes = [C.c_void_p, C.c_uint32]
        L.azr_samples_copy_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.azr_selfplay_run.argtypes = [C.c_void_p, C.c_int]
        L.azr_samples_drain.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.azr_samples_device_view.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.azr_mcts_pick.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.azr_mcts_leaves.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.azr_mcts_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.azr_mcts_root_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.azr_profile_last_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.azr_debug_tower_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        for name in ("azr_engine_destroy", "azr_engine_games", "azr_mcts_clear", "azr_mcts_trim", "azr_mcts_simulate",
                     "azr_mcts_begin", "azr_device_synchronize"):
            getattr(L, name).argtypes = [C.c_void_p]
        for name in ("azr_engine_new_games", "azr_engine_set_states", "azr_engine_get_states", "azr_engine_set_rng",
                     "azr_engine_get_rng", "azr_engine_valid_moves", "azr_engine_status", "azr_engine_encode",
                     "azr_mcts_policy", "azr_selfplay_counters"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p]
        L.azr_engine_make_moves.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.azr_arena_start.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32]
        L.azr_arena_run.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.azr_arena_set_opponent_net.argtypes = [C.c_void_p, C.c_void_p]
        L.azr_arena_set_opponent_search.argtypes = [C.c_void_p, C.c_int, C.c_float]
        L.azr_arena_set_gumbel.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int]
        L.azr_arena_collect_samples.argtypes = [C.c_void_p, C.c_int]
        L.azr_arena_collect_scripted_samples.argtypes = [C.c_void_p, C.c_int]
        L.azr_arena_results.argtypes = [C.c_void_p, C.c_void_p]
        L.azr_arena_log.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.azr_mcts_set_root_noise.argtypes = [C.c_void_p, C.c_void_p]
        L.azr_selfplay_set_dirichlet.argtypes = [C.c_void_p, C.c_float, C.c_uint32]
        L.azr_mcts_root_noise.argtypes = [C.c_void_p, C.c_void_p]
        L.azr_debug_root_noise.argtypes = [C.c_void_p, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.azr_selfplay_set_playout_cap.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_uint32]
        L.azr_selfplay_decision_kind.argtypes = [C.c_void_p, C.c_void_p]
        L.azr_debug_playout_cap.argtypes = [C.c_void_p, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.azr_mcts_set_forced_playouts.argtypes = [C.c_void_p, C.c_float]
        L.azr_mcts_pruned_policy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.azr_selfplay_set_forced_playouts.argtypes = [C.c_void_p, C.c_float, C.c_int]
        L.azr_mcts_set_simulations.argtypes = [C.c_void_p, C.c_int]
        L.azr_selfplay_start_games_from_states.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64]
        L.azr_selfplay_set_surprise_weighting.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_uint32]
        L.azr_debug_surprise_weights.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.azr_selfplay_set_value_mix.argtypes = [C.c_void_p, C.c_float]
        L.azr_mcts_root_value.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.azr_debug_value_mix.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p]
        L.azr_selfplay_set_resign.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_float, C.c_uint32]
        L.azr_selfplay_resign_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.azr_selfplay_resign_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.azr_debug_resign.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.azr_selfplay_set_gumbel.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_uint32]
        L.azr_mcts_set_gumbel.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float]
        L.azr_mcts_set_root_gumbel.argtypes = [C.c_void_p, C.c_void_p]
        L.azr_mcts_root_gumbel.argtypes = [C.c_void_p, C.c_void_p]
        L.azr_mcts_gumbel_policy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.azr_mcts_gumbel_pick.argtypes = [C.c_void_p, C.c_void_p]
        L.azr_debug_root_gumbel.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.azr_debug_gumbel_select.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float] + [C.c_void_p] * 9 + [C.c_int, C.c_void_p, C.c_void_p]
        L.azr_selfplay_set_gumbel_tree.argtypes = [C.c_void_p, C.c_int]
        L.azr_mcts_set_gumbel_tree.argtypes = [C.c_void_p, C.c_int]
        L.azr_debug_gumbel_tree_select.argtypes = [C.c_void_p, C.c_float, C.c_float] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_void_p]
        L.azr_mcts_node_stats.argtypes = [C.c_void_p] * 8
        L.azr_debug_exp32.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _libs[test_hooks] = L
        if not test_hooks:
            _lib = L
    return _libs[test_hooks]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Engine:
    """One handle = one GPU = G concurrent games.  Method names follow the reference seams:
    State / UtilityNN (rules), AlphaZeroNNId (net), AlphaZeroMCTS (search), trainer move loop (self-play)."""

    def __init__(self, games, blocks=20, sims=32, dtype=NET_BF16, device=0, threads=1, test_hooks=False, **kw):
        """threads = THREADS_PER_MCTS.  The C default (azr_default_settings) is the reference's 2; this binding defaults
        to 1, the only value at which the reference's search is deterministic and the parity tests are bit-exact
        against `-t 1` semantics; tests of the T-thread schedule pass it explicitly.  test_hooks: the handle lives in
        libazr_hip_test.so (tests only: the build whose environment switches select other formulations)."""
        self.L = load_library(test_hooks)
        s = Settings()
        self.L.azr_default_settings(C.byref(s))
        s.device, s.games, s.blocks, s.mcts_simulations, s.net_dtype = device, games, blocks, sims, dtype
        s.mcts_threads = threads
        self.T = threads
        for k, v in kw.items():
            if not hasattr(s, k):
                raise TypeError(f"unknown setting {k}")
            setattr(s, k, v)
        self.settings = s
        self.G = games
        self.blocks = blocks
        self.h = C.c_void_p()
        rc = self.L.azr_engine_create(C.byref(s), C.byref(self.h))
        if rc:  # *out is NULL on failure; the reason is kept per thread
            self.h = None
            raise AzrError(rc, self.L.azr_last_error(None).decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.azr_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise AzrError(rc, self.L.azr_last_error(self.h).decode())

    # ---- rules
    def new_games(self, seeds):
        seeds = np.ascontiguousarray(seeds, np.uint32)
        assert seeds.shape == (self.G,)
        self._chk(self.L.azr_engine_new_games(self.h, _p(seeds)))

    def set_states(self, data160):
        d = np.ascontiguousarray(data160, np.uint8)
        assert d.shape == (self.G, 160)
        self._chk(self.L.azr_engine_set_states(self.h, _p(d)))

    def get_states(self):
        d = np.zeros((self.G, 160), np.uint8)
        self._chk(self.L.azr_engine_get_states(self.h, _p(d)))
        return d

    def set_rng(self, x):
        x = np.ascontiguousarray(x, np.uint32)
        assert x.shape == (self.G,)
        self._chk(self.L.azr_engine_set_rng(self.h, _p(x)))

    def get_rng(self):
        x = np.zeros(self.G, np.uint32)
        self._chk(self.L.azr_engine_get_rng(self.h, _p(x)))
        return x

    def valid_moves(self):
        m = np.zeros(self.G, np.uint64)
        self._chk(self.L.azr_engine_valid_moves(self.h, _p(m)))
        return m

    def make_moves(self, moves):
        mv = np.ascontiguousarray(moves, np.uint8)
        assert mv.shape == (self.G,)
        rc = np.zeros(self.G, np.uint8)
        self._chk(self.L.azr_engine_make_moves(self.h, _p(mv), _p(rc)))
        return rc

    def status(self):
        s = np.zeros(self.G, np.int8)
        self._chk(self.L.azr_engine_status(self.h, _p(s)))
        return s

    def encode(self):
        e = np.zeros((self.G, 88), np.uint8)
        self._chk(self.L.azr_engine_encode(self.h, _p(e)))
        return e

    # ---- net
    def param_count(self):
        return self.L.azr_nn_param_count(self.blocks)

    def init_random(self, seed=20260002):
        self._chk(self.L.azr_nn_init_random(self.h, seed))

    def set_weights(self, flat):
        f = np.ascontiguousarray(flat, np.float32)
        self._chk(self.L.azr_nn_set_weights(self.h, _p(f), f.size))

    def get_weights(self):
        f = np.zeros(self.param_count(), np.float32)
        self._chk(self.L.azr_nn_get_weights(self.h, _p(f), f.size))
        return f

    def save(self, path):
        self._chk(self.L.azr_nn_save(self.h, path.encode()))

    def load(self, path):
        self._chk(self.L.azr_nn_load(self.h, path.encode()))

    def predict(self, in88):
        x = np.ascontiguousarray(in88, np.uint8)
        n = x.shape[0]
        assert x.shape == (n, 88)
        pi = np.zeros((n, 43), np.float32)
        v = np.zeros(n, np.float32)
        self._chk(self.L.azr_nn_predict(self.h, _p(x), n, _p(pi), _p(v)))
        return pi, v

    def train(self, rec265, epochs, batch_size=512, rng_state=None):
        """AlphaZeroNNId::train: returns ([(loss_pi, loss_v)] per epoch, engine state after the shuffles)"""
        r = np.ascontiguousarray(rec265, np.uint8).reshape(-1, 265)
        lp = np.zeros(max(epochs, 1), np.float32)
        lv = np.zeros(max(epochs, 1), np.float32)
        st = np.array([rng_state if rng_state is not None else 1], np.uint32)
        self._chk(self.L.azr_nn_train(self.h, _p(r), len(r), epochs, batch_size, _p(st) if rng_state is not None else None,
                                      _p(lp), _p(lv)))
        return [(float(lp[e]), float(lv[e])) for e in range(epochs)], int(st[0])

    def dp_init(self, rank, world, id128):
        """azr_dp_init: this handle's RCCL communicator (collective over the `world` processes); id128 = dp_unique_id() of rank 0"""
        b = (C.c_uint8 * 128).from_buffer_copy(bytes(id128))
        self._chk(self.L.azr_dp_init(self.h, rank, world, b))

    def dp_shutdown(self):
        self._chk(self.L.azr_dp_shutdown(self.h))

    def train_dp(self, rec265, epochs, allreduce, rank, world, batch_size=512, rng_state=None):
        """azr_nn_train_dp: this rank's share of a data-parallel AlphaZeroNNId::train.  allreduce(device_ptr, count, dtype)
        sums a device buffer over the ranks in place (dtype 0 = float32, 1 = float64); see shard.make_allreduce.  allreduce = None:
        the handle's own RCCL communicator (dp_init), every sum in stream order."""
        if allreduce is None:
            r = np.ascontiguousarray(rec265, np.uint8).reshape(-1, 265)
            lp = np.zeros(max(epochs, 1), np.float32)
            lv = np.zeros(max(epochs, 1), np.float32)
            st = np.array([rng_state if rng_state is not None else 1], np.uint32)
            self._chk(self.L.azr_nn_train_dp(self.h, _p(r), len(r), epochs, batch_size, _p(st) if rng_state is not None else None, rank, world,
                                             C.cast(None, ALLREDUCE_FN), None, _p(lp), _p(lv)))
            return [(float(lp[e]), float(lv[e])) for e in range(epochs)], int(st[0])
        r = np.ascontiguousarray(rec265, np.uint8).reshape(-1, 265)
        lp = np.zeros(max(epochs, 1), np.float32)
        lv = np.zeros(max(epochs, 1), np.float32)
        st = np.array([rng_state if rng_state is not None else 1], np.uint32)

        def cb(ctx, ptr, count, dtype):
            try:
                allreduce(ptr, count, dtype)
                return 0
            except Exception as e:   # never let an exception cross the C frame
                self._dp_error = e
                return 1

        fn = ALLREDUCE_FN(cb)
        self._dp_error = None
        rc = self.L.azr_nn_train_dp(self.h, _p(r), len(r), epochs, batch_size, _p(st) if rng_state is not None else None, rank, world,
                                    fn, None, _p(lp), _p(lv))
        if rc and self._dp_error is not None:
            raise self._dp_error
        self._chk(rc)
        return [(float(lp[e]), float(lv[e])) for e in range(epochs)], int(st[0])

    def train_batch(self, rec265):
        """one optimiser step on exactly these records; returns (loss_pi, loss_v)"""
        r = np.ascontiguousarray(rec265, np.uint8).reshape(-1, 265)
        l = np.zeros(2, np.float32)
        self._chk(self.L.azr_nn_train_batch(self.h, _p(r), len(r), _p(l[0:1]), _p(l[1:2])))
        return float(l[0]), float(l[1])

    def validate(self, rec265, batch_size=512, per_record=False):
        """azr_nn_validate: the cross-validation loss of these records in inference mode (BN on the moving statistics, no update):
        (loss_pi, loss_v) averaged over the floor(n / batch_size) batches (NaN when n < batch_size); per_record=True adds the
        per-record cross-entropy and squared error of the evaluated records"""
        r = np.ascontiguousarray(rec265, np.uint8).reshape(-1, 265)
        l = np.zeros(2, np.float32)
        m = (len(r) // batch_size) * batch_size if batch_size > 0 else 0
        rp = np.zeros(max(m, 1), np.float32)
        rv = np.zeros(max(m, 1), np.float32)
        self._chk(self.L.azr_nn_validate(self.h, _p(r) if len(r) else None, len(r), batch_size, _p(l[0:1]), _p(l[1:2]),
                                         _p(rp) if per_record else None, _p(rv) if per_record else None))
        if per_record:
            return float(l[0]), float(l[1]), rp[:m], rv[:m]
        return float(l[0]), float(l[1])

    def train_grads(self):
        g = np.zeros(self.L.azr_nn_param_count(self.settings.blocks), np.float32)
        self._chk(self.L.azr_nn_train_grads(self.h, _p(g), g.size))
        return g

    def train_reset(self):
        self._chk(self.L.azr_nn_train_reset(self.h))

    def train_set_options(self, **kw):
        """azr_nn_train_set_options: the defaults (azr_default_train_options) with the given fields of azr_train_options replaced;
        lr_schedule is LR_CONSTANT / LR_COSINE / LR_STEP or its name.  Read when the next training call is entered."""
        o = TrainOptions()
        self.L.azr_default_train_options(C.byref(o))
        for k, v in kw.items():
            if k not in dict(TrainOptions._fields_):
                raise TypeError(f"unknown training option {k}")
            setattr(o, k, LR_SCHEDULES[v] if k == "lr_schedule" and isinstance(v, str) else v)
        self._chk(self.L.azr_nn_train_set_options(self.h, C.byref(o)))

    def train_options(self):
        """azr_nn_train_get_options as a dict of azr_train_options' fields"""
        o = TrainOptions()
        self._chk(self.L.azr_nn_train_get_options(self.h, C.byref(o)))
        return o.as_dict()

    def train_stats(self):
        """azr_nn_train_stats of the last step as a dict of azr_train_stats' fields (AZR_E_STATE before the first step)"""
        s = TrainStats()
        self._chk(self.L.azr_nn_train_stats(self.h, C.byref(s)))
        return s.as_dict()

    def get_ema_weights(self):
        """azr_nn_get_ema_weights: the EMA vector in AZRW layout (AZR_E_STATE while there is none)"""
        f = np.zeros(self.param_count(), np.float32)
        self._chk(self.L.azr_nn_get_ema_weights(self.h, _p(f), f.size))
        return f

    # ---- search
    def mcts_clear(self):
        self._chk(self.L.azr_mcts_clear(self.h))

    def mcts_trim(self):
        self._chk(self.L.azr_mcts_trim(self.h))

    def simulate(self):
        self._chk(self.L.azr_mcts_simulate(self.h))

    def mcts_begin(self):
        self._chk(self.L.azr_mcts_begin(self.h))

    def mcts_leaves(self):
        x = np.zeros((self.G * self.T, 88), np.uint8)      # slot = g * T + k
        need = np.zeros(self.G * self.T, np.uint8)
        act = C.c_int(0)
        self._chk(self.L.azr_mcts_leaves(self.h, _p(x), _p(need), C.byref(act)))
        return x, need.astype(bool), act.value

    def mcts_apply(self, pi, v):
        pi = np.ascontiguousarray(pi, np.float32)
        v = np.ascontiguousarray(v, np.float32)
        assert pi.shape == (self.G * self.T, 43) and v.shape == (self.G * self.T,)
        self._chk(self.L.azr_mcts_apply(self.h, _p(pi), _p(v)))

    def root_stats(self):
        n = np.zeros((self.G, 43), np.uint32)
        q = np.zeros((self.G, 43), np.float32)
        p = np.zeros((self.G, 43), np.float32)
        self._chk(self.L.azr_mcts_root_stats(self.h, _p(n), _p(q), _p(p)))
        return n, q, p

    def node_stats(self, data160):
        """the rows of the node of state g of data160 [G, 160] in game g's tree: (N, act, Q, P [G, 43], vhat [G], found [G] bool); zero
        rows where the state is not in the tree.  Reads only."""
        d = np.ascontiguousarray(data160, np.uint8)
        assert d.shape == (self.G, 160)
        n, act = np.zeros((self.G, 43), np.uint32), np.zeros((self.G, 43), np.uint32)
        q, p = np.zeros((self.G, 43), np.float32), np.zeros((self.G, 43), np.float32)
        vhat, found = np.zeros(self.G, np.float32), np.zeros(self.G, np.uint8)
        self._chk(self.L.azr_mcts_node_stats(self.h, _p(d), _p(n), _p(act), _p(q), _p(p), _p(vhat), _p(found)))
        return n, act, q, p, vhat, found.astype(bool)

    def policy(self):
        pi = np.zeros((self.G, 43), np.float32)
        self._chk(self.L.azr_mcts_policy(self.h, _p(pi)))
        return pi

    def pick(self, sample=False):
        m = np.zeros(self.G, np.uint8)
        self._chk(self.L.azr_mcts_pick(self.h, int(sample), _p(m)))
        return m

    # ---- root noise (this engine's own; off = the reference's constant)
    def set_root_noise(self, eta):
        """host-stepped searches: eta [G, 43] replaces DIR_NOISE_VALUE in the first selection of every descent, used as given;
        None = off"""
        if eta is None:
            self._chk(self.L.azr_mcts_set_root_noise(self.h, None))
            return
        e = np.ascontiguousarray(eta, np.float32)
        assert e.shape == (self.G, MOVES)
        self._chk(self.L.azr_mcts_set_root_noise(self.h, _p(e)))

    def selfplay_set_dirichlet(self, alpha, noise_seed=0):
        """device self-play: Dirichlet(alpha) over every new root's legal moves (alpha <= 0 = off); read by selfplay_start*"""
        self._chk(self.L.azr_selfplay_set_dirichlet(self.h, float(alpha), int(noise_seed)))

    def root_noise(self):
        """the vector in force at each game's current root, [G, 43]; zeros where none"""
        e = np.zeros((self.G, MOVES), np.float32)
        self._chk(self.L.azr_mcts_root_noise(self.h, _p(e)))
        return e

    def debug_root_noise(self, alpha, noise_seed, game_seed, decision, valid):
        """the sampler alone: one vector per (game_seed[i], decision[i], valid[i]) -> [n, 43]"""
        s = np.ascontiguousarray(game_seed, np.uint32)
        d = np.ascontiguousarray(decision, np.uint32)
        v = np.ascontiguousarray(valid, np.uint64)
        assert s.ndim == 1 and s.shape == d.shape == v.shape
        e = np.zeros((len(s), MOVES), np.float32)
        self._chk(self.L.azr_debug_root_noise(self.h, float(alpha), int(noise_seed), _p(s), _p(d), _p(v), len(s), _p(e)))
        return e

    # ---- playout cap (this engine's own; off = every decision gets the whole budget and a record)
    def selfplay_set_playout_cap(self, full_prob, fast_simulations, cap_seed=0):
        """device self-play: a decision is full (mcts_simulations, sampled root noise, a record) with probability full_prob by a coin of
        (cap_seed, game seed, decision), else fast (fast_simulations, the constant noise, no record); full_prob >= 1 or
        fast_simulations <= 0 = off; read by selfplay_start*"""
        self._chk(self.L.azr_selfplay_set_playout_cap(self.h, float(full_prob), int(fast_simulations), int(cap_seed)))

    def decision_kind(self):
        """1 = full, 0 = fast for each slot's current decision, [G] uint8; all 1 without a cap or outside self-play"""
        k = np.zeros(self.G, np.uint8)
        self._chk(self.L.azr_selfplay_decision_kind(self.h, _p(k)))
        return k

    def debug_playout_cap(self, full_prob, cap_seed, game_seed, decision):
        """the coin alone, on the device: 1 = full, 0 = fast per (game_seed[i], decision[i]) -> [n] uint8"""
        s = np.ascontiguousarray(game_seed, np.uint32)
        d = np.ascontiguousarray(decision, np.uint32)
        assert s.ndim == 1 and s.shape == d.shape
        o = np.zeros(len(s), np.uint8)
        self._chk(self.L.azr_debug_playout_cap(self.h, float(full_prob), int(cap_seed), _p(s), _p(d), len(s), _p(o)))
        return o

    # ---- forced playouts and policy target pruning (this engine's own; off = the search and the records above)
    def set_forced_playouts(self, k):
        """host-stepped searches: at path depth 0 a tried root move is selected until it has sqrt(k * noiseP * sumN) visits;
        k <= 0 = off; holds until set again or selfplay_start*"""
        self._chk(self.L.azr_mcts_set_forced_playouts(self.h, float(k)))

    def pruned_policy(self):
        """(pi [G, 43], N' [G, 43]) of the last search's roots under policy target pruning with the factor and vector in force;
        policy() stays the unpruned one"""
        pi = np.zeros((self.G, MOVES), np.float32)
        n = np.zeros((self.G, MOVES), np.uint32)
        self._chk(self.L.azr_mcts_pruned_policy(self.h, _p(pi), _p(n)))
        return pi, n

    def selfplay_set_forced_playouts(self, k, prune=False):
        """device self-play: forced playouts in every full decision, and with prune the pruned policy in the records; k <= 0 = off;
        read by selfplay_start*"""
        self._chk(self.L.azr_selfplay_set_forced_playouts(self.h, float(k), int(bool(prune))))

    def set_simulations(self, simulations):
        """host-stepped searches: the budget per search, within [threads, sims]; <= 0 = the settings' own"""
        self._chk(self.L.azr_mcts_set_simulations(self.h, int(simulations)))

    # ---- policy surprise weighting of the records (this engine's own; off = every record of a finished game is written once)
    def selfplay_set_surprise_weighting(self, share, max_weight=4.0, seed=0):
        """device self-play: a finished game's n records share the weight n, `share` of it in proportion to KL(pi || prior), each weight
        capped at max_weight; record r is written floor(w) or ceil(w) times by a coin of (seed, game seed, r); share <= 0 = off; read by
        selfplay_start*"""
        self._chk(self.L.azr_selfplay_set_surprise_weighting(self.h, float(share), float(max_weight), int(seed)))

    def debug_surprise_weights(self, share, max_weight, seed, pi, prior, valid, game_len, game_seed):
        """the rule alone, on the device: pi, prior [rows, 43] and valid [rows] hold the games' records one game after the other
        (rows = sum(game_len)) -> (kl, w, copies), each [rows]"""
        pi = np.ascontiguousarray(pi, np.float32)
        prior = np.ascontiguousarray(prior, np.float32)
        v = np.ascontiguousarray(valid, np.uint64)
        n = np.ascontiguousarray(game_len, np.uint32)
        s = np.ascontiguousarray(game_seed, np.uint32)
        rows = int(n.sum())
        assert pi.shape == prior.shape == (rows, MOVES) and v.shape == (rows,) and n.ndim == 1 and n.shape == s.shape
        kl, w, c = np.zeros(rows, np.float32), np.zeros(rows, np.float32), np.zeros(rows, np.uint32)
        self._chk(self.L.azr_debug_surprise_weights(self.h, float(share), float(max_weight), int(seed), _p(pi), _p(prior), _p(v), _p(n), _p(s),
                                                    len(n), _p(kl), _p(w), _p(c)))
        return kl, w, c

    # ---- value mix of the records (this engine's own; off = every record carries the bare game outcome z)
    def selfplay_set_value_mix(self, q_share):
        """device self-play: a finished game's records carry z' = (1 - q_share) * z + q_share * q, q the visit-weighted mean of the
        root's Q at the recorded decision; q_share <= 0 = off; read by selfplay_start*"""
        self._chk(self.L.azr_selfplay_set_value_mix(self.h, float(q_share)))

    def root_value(self):
        """(q [G] float32, has_q [G] bool) of the last search's roots, by the device function the self-play step uses"""
        q, has = np.zeros(self.G, np.float32), np.zeros(self.G, np.uint8)
        self._chk(self.L.azr_mcts_root_value(self.h, _p(q), _p(has)))
        return q, has.astype(bool)

    def debug_value_mix(self, q_share, N, Q, valid, z):
        """the rule alone, on the device: N, Q [rows, 43], valid, z [rows] -> (q, has_q, z'), each [rows]"""
        N = np.ascontiguousarray(N, np.uint32)
        Q = np.ascontiguousarray(Q, np.float32)
        v = np.ascontiguousarray(valid, np.uint64)
        z = np.ascontiguousarray(z, np.float32)
        rows = len(z)
        assert N.shape == Q.shape == (rows, MOVES) and v.shape == (rows,)
        q, has, zz = np.zeros(rows, np.float32), np.zeros(rows, np.uint8), np.zeros(rows, np.float32)
        self._chk(self.L.azr_debug_value_mix(self.h, float(q_share), _p(N), _p(Q), _p(v), _p(z), rows, _p(q), _p(has), _p(zz)))
        return q, has.astype(bool), zz

    # ---- resignation with a no-resign holdout (this engine's own; off = every game is played to its end)
    def selfplay_set_resign(self, q_resign, streak, holdout_share=0.1, seed=0):
        """device self-play: a player whose root value q stays below q_resign for `streak` of its own recorded decisions in a row gives
        the game up; a game held out by the coin of (seed, game seed, holdout_share) plays on and counts in the holdout statistics;
        streak <= 0 = off; read by selfplay_start*"""
        self._chk(self.L.azr_selfplay_set_resign(self.h, float(q_resign), int(streak), float(holdout_share), int(seed)))

    def selfplay_resign_stats(self):
        """dict(resigned, holdout_games, holdout_would_resign, holdout_not_lost) since the self-play counters were reset"""
        s = ResignStats()
        self._chk(self.L.azr_selfplay_resign_stats(self.h, C.byref(s)))
        return s.as_dict()

    def selfplay_resign_state(self):
        """(run [G, 2] uint8, first [G] uint8 with 255 = none, holdout [G] bool) of the slots' running games"""
        run, first, hold = np.zeros((self.G, 2), np.uint8), np.zeros(self.G, np.uint8), np.zeros(self.G, np.uint8)
        self._chk(self.L.azr_selfplay_resign_state(self.h, _p(run), _p(first), _p(hold)))
        return run, first, hold.astype(bool)

    def debug_resign(self, q_resign, streak, holdout_share, seed, q, has_q, player, game_len, game_seed):
        """the rule alone, on the device: q, has_q, player [rows] hold the games' decisions one game after the other
        (rows = sum(game_len)) -> (resign_row [games] int32 with -1 = never, resigner [games] uint8 with 255 = nobody, holdout [games] bool)"""
        q = np.ascontiguousarray(q, np.float32)
        hq = np.ascontiguousarray(has_q, np.uint8)
        pl = np.ascontiguousarray(player, np.uint8)
        n = np.ascontiguousarray(game_len, np.uint32)
        s = np.ascontiguousarray(game_seed, np.uint32)
        rows = int(n.sum())
        assert q.shape == hq.shape == pl.shape == (rows,) and n.ndim == 1 and n.shape == s.shape
        row, who, hold = np.zeros(len(n), np.int32), np.zeros(len(n), np.uint8), np.zeros(len(n), np.uint8)
        self._chk(self.L.azr_debug_resign(self.h, float(q_resign), int(streak), float(holdout_share), int(seed), _p(q), _p(hq), _p(pl),
                                          _p(n), _p(s), len(n), _p(row), _p(who), _p(hold)))
        return row, who, hold.astype(bool)

    # ---- Gumbel root search with sequential halving (this engine's own; off = PUCT at the root and the visit distribution as pi)
    def selfplay_set_gumbel(self, m, c_visit=50.0, c_scale=0.5, seed=0):
        """device self-play: every root considers its m best moves by g + logit (g a Gumbel vector of (seed, game seed, decision)),
        spends the budget on them by sequential halving, plays the most visited and records softmax(logit + sigma(completed Q));
        m = 0 = off; read by selfplay_start*, which refuses it together with Dirichlet noise, a playout cap or forced playouts"""
        self._chk(self.L.azr_selfplay_set_gumbel(self.h, int(m), float(c_visit), float(c_scale), int(seed)))

    def set_gumbel(self, m, c_visit=50.0, c_scale=0.5):
        """host-stepped searches: the same search under the vector of set_root_gumbel; m = 0 = off; clears the trees when it toggles"""
        self._chk(self.L.azr_mcts_set_gumbel(self.h, int(m), float(c_visit), float(c_scale)))

    def set_root_gumbel(self, g):
        """g [G, 43] for the searches that follow, used as given; None = zeros"""
        if g is None:
            self._chk(self.L.azr_mcts_set_root_gumbel(self.h, None))
            return
        g = np.ascontiguousarray(g, np.float32)
        assert g.shape == (self.G, MOVES)
        self._chk(self.L.azr_mcts_set_root_gumbel(self.h, _p(g)))

    def root_gumbel(self):
        """the Gumbel vector in force at each game's current root, [G, 43]; zeros where none"""
        g = np.zeros((self.G, MOVES), np.float32)
        self._chk(self.L.azr_mcts_root_gumbel(self.h, _p(g)))
        return g

    def gumbel_policy(self):
        """(pi [G, 43], completed Q [G, 43]) of the last search's roots, as a self-play decision records them"""
        pi, q = np.zeros((self.G, MOVES), np.float32), np.zeros((self.G, MOVES), np.float32)
        self._chk(self.L.azr_mcts_gumbel_policy(self.h, _p(pi), _p(q)))
        return pi, q

    def gumbel_pick(self):
        """the Gumbel decision's move of every game, [G] uint8; nothing is drawn"""
        m = np.zeros(self.G, np.uint8)
        self._chk(self.L.azr_mcts_gumbel_pick(self.h, _p(m)))
        return m

    def debug_root_gumbel(self, seed, game_seed, decision, valid, greedy):
        """the draw alone: one vector per (game_seed[i], decision[i], valid[i], greedy[i]) -> [n, 43]"""
        s = np.ascontiguousarray(game_seed, np.uint32)
        d = np.ascontiguousarray(decision, np.uint32)
        v = np.ascontiguousarray(valid, np.uint64)
        gr = np.ascontiguousarray(greedy, np.uint8)
        assert s.ndim == 1 and s.shape == d.shape == v.shape == gr.shape
        g = np.zeros((len(s), MOVES), np.float32)
        self._chk(self.L.azr_debug_root_gumbel(self.h, int(seed), _p(s), _p(d), _p(v), _p(gr), len(s), _p(g)))
        return g

    def debug_gumbel_select(self, m, n, c_visit, c_scale, N, N0, act, Q, P, g, vhat, valid, claim):
        """the root-level selection alone on synthetic rows: N, N0, act, Q, P, g [rows, 43], vhat, valid, claim [rows] -> (move, cv)"""
        N, N0, act = (np.ascontiguousarray(a, np.uint32) for a in (N, N0, act))
        Q, P, g, vhat = (np.ascontiguousarray(a, np.float32) for a in (Q, P, g, vhat))
        v = np.ascontiguousarray(valid, np.uint64)
        c = np.ascontiguousarray(claim, np.uint32)
        rows = len(v)
        assert N.shape == N0.shape == act.shape == Q.shape == P.shape == g.shape == (rows, MOVES) and vhat.shape == c.shape == (rows,)
        mv, cv = np.zeros(rows, np.uint8), np.zeros(rows, np.uint32)
        self._chk(self.L.azr_debug_gumbel_select(self.h, int(m), int(n), float(c_visit), float(c_scale), _p(N), _p(N0), _p(act), _p(Q), _p(P),
                                                 _p(g), _p(vhat), _p(v), _p(c), rows, _p(mv), _p(cv)))
        return mv, cv

    def selfplay_set_gumbel_tree(self, on):
        """device self-play under selfplay_set_gumbel: 1 = below the root every node spends its visits in proportion to
        softmax(logit + sigma(completed Q)) of its own rows, 0 (default) = PUCT there; read by selfplay_start*"""
        self._chk(self.L.azr_selfplay_set_gumbel_tree(self.h, int(on)))

    def set_gumbel_tree(self, on):
        """host-stepped searches under set_gumbel: the same switch; the trees stay"""
        self._chk(self.L.azr_mcts_set_gumbel_tree(self.h, int(on)))

    def debug_gumbel_tree_select(self, c_visit, c_scale, N, act, Q, P, vhat, valid):
        """the selection below the root alone on synthetic rows: N, act, Q, P [rows, 43], vhat, valid [rows] -> (move, score [rows, 43])"""
        N, act = (np.ascontiguousarray(a, np.uint32) for a in (N, act))
        Q, P, vhat = (np.ascontiguousarray(a, np.float32) for a in (Q, P, vhat))
        v = np.ascontiguousarray(valid, np.uint64)
        rows = len(v)
        assert N.shape == act.shape == Q.shape == P.shape == (rows, MOVES) and vhat.shape == (rows,)
        mv, score = np.zeros(rows, np.uint8), np.zeros((rows, MOVES), np.float32)
        self._chk(self.L.azr_debug_gumbel_tree_select(self.h, float(c_visit), float(c_scale), _p(N), _p(act), _p(Q), _p(P), _p(vhat), _p(v), rows,
                                                      _p(mv), _p(score)))
        return mv, score

    def debug_exp32(self, x):
        """the engine's exponential alone, on the device"""
        x = np.ascontiguousarray(x, np.float32)
        out = np.zeros(x.shape, np.float32)
        self._chk(self.L.azr_debug_exp32(self.h, _p(x), x.size, _p(out)))
        return out

    # ---- self-play
    def selfplay_start(self, base_seed=20260001):
        self._chk(self.L.azr_selfplay_start(self.h, base_seed))

    def selfplay_start_games(self, base_seed, games):
        """exactly `games` games (seeds base_seed .. base_seed + games - 1), each played to its end"""
        self._chk(self.L.azr_selfplay_start_games(self.h, base_seed, games))

    def selfplay_start_from_states(self, base_seed=20260001):
        """self-play goes on from the states / RNG streams set with set_states / set_rng"""
        self._chk(self.L.azr_selfplay_start_from_states(self.h, base_seed))

    def selfplay_start_games_from_states(self, base_seed, games):
        """the games of slots 0 .. min(games, G) - 1 go on from the states / RNG streams set; no other game starts while games <= G"""
        self._chk(self.L.azr_selfplay_start_games_from_states(self.h, base_seed, games))

    def selfplay_run(self, passes):
        self._chk(self.L.azr_selfplay_run(self.h, passes))

    def counters(self):
        c = Counters()
        self._chk(self.L.azr_selfplay_counters(self.h, C.byref(c)))
        return c.as_dict()

    def drain(self, cap=None):
        """the first `cap` buffered records (default: all); what does not fit stays buffered"""
        if cap is None:
            cap = max(1, self.samples_device_view()[1])
        buf = np.empty((cap, RECORD_BYTES), np.uint8)
        n = C.c_size_t(0)
        self._chk(self.L.azr_samples_drain(self.h, _p(buf), cap, C.byref(n)))
        return buf[:n.value].copy()

    def discard_samples(self):
        self._chk(self.L.azr_samples_drain(self.h, None, 0, None))

    def samples_copy_device(self, dst_ptr, cap):
        """copy up to `cap` buffered records to device memory at dst_ptr (engine stream); returns the count"""
        n = C.c_size_t(0)
        self._chk(self.L.azr_samples_copy_device(self.h, C.c_void_p(dst_ptr), cap, C.byref(n)))
        return n.value

    def samples_device_view(self):
        ptr = C.c_void_p()
        n = C.c_size_t(0)
        self._chk(self.L.azr_samples_device_view(self.h, C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    def tower_plan(self, n):
        """(boards per workgroup, workgroups) of a bf16 net launch of n boards"""
        nb, w = C.c_int(0), C.c_int(0)
        self._chk(self.L.azr_debug_tower_plan(self.h, n, C.byref(nb), C.byref(w)))
        return nb.value, w.value

    def profile_last_run(self):
        a, b, k = C.c_float(0), C.c_float(0), C.c_int(0)
        self._chk(self.L.azr_profile_last_run(self.h, C.byref(a), C.byref(b), C.byref(k)))
        return dict(net_ms=a.value, tree_ms=b.value, launches=k.value)

    # ---- arena (GameGroup::playGames)
    def arena_start(self, player1, player2, games, per_slot_cap=0, mirror=True, base_seed=20260001):
        """mirror: False / True (= MIRROR_SEQUENTIAL, the reference's thread-per-pair form) / MIRROR_CONCURRENT (a pair's two games at
        the same time on slots 2j, 2j + 1)"""
        self._chk(self.L.azr_arena_start(self.h, player1, player2, games, per_slot_cap, int(mirror), base_seed))

    def arena_set_opponent(self, other):
        """the network of PLAYER_ALPHAZERO_B = `other`'s: an Engine on the same device with at least this one's leaf slots (games x
        threads), or None to detach.  Its blocks and dtype may differ from this Engine's (a 5-block net against a 20-block one, bf16
        against f32x).  Pairings of NET_BF16 / NET_F16 / NET_F32X run without a host read-back per pass up to 256 leaf slots; an arena
        with a NET_F32 side reads the leaf counts back every pass."""
        self._chk(self.L.azr_arena_set_opponent_net(self.h, other.h if other is not None else None))
        self._opponent = other   # keep it alive

    def arena_set_opponent_search(self, sims=None, hp=None):
        """the search budget of PLAYER_ALPHAZERO_B: its simulations per decision and its PUCT constant (None = this Engine's own).  Holds
        until it is set again or arena_set_opponent(None); refused while an arena runs, below `threads`, and above what the node pool
        holds (16 * (sims + 1) nodes: create the Engine with node_capacity for the larger of the two budgets)."""
        self._chk(self.L.azr_arena_set_opponent_search(self.h, -1 if sims is None else int(sims), -1.0 if hp is None else float(hp)))

    def arena_set_gumbel(self, player, m, c_visit=50.0, c_scale=0.5, tree=0):
        """the search of one AlphaZero player of this Engine's arenas (PLAYER_ALPHAZERO or PLAYER_ALPHAZERO_B): m > 0 = the Gumbel root
        search with sequential halving over m moves, deterministic (g = 0), tree = 1 with the improved-policy selection below the root;
        m = 0 = PUCT (the default).  With arena_collect_samples its records carry the improved policy.  Holds until it is set again
        (player B's also until arena_set_opponent(None)); refused while an arena runs, and arena_start refuses a Gumbel side under
        arena_collect_scripted_samples."""
        self._chk(self.L.azr_arena_set_gumbel(self.h, int(player), int(m), float(c_visit), float(c_scale), int(tree)))

    def arena_collect_samples(self, on=True):
        self._chk(self.L.azr_arena_collect_samples(self.h, int(on)))

    def arena_collect_scripted_samples(self, on=True):
        """ScriptPlayer / RandomPlayer record one-hot (s, move) samples (include/azr.h); set before arena_start, and drain
        after every arena_run: a run may return unfinished while slots wait for ring room"""
        self._chk(self.L.azr_arena_collect_scripted_samples(self.h, int(on)))

    def arena_run(self, passes):
        fin = C.c_int(0)
        self._chk(self.L.azr_arena_run(self.h, passes, C.byref(fin)))
        return bool(fin.value)

    def arena_results(self):
        r = GameResults()
        self._chk(self.L.azr_arena_results(self.h, C.byref(r)))
        return r.as_dict()

    def arena_log(self):
        n = np.zeros(self.G, np.int32)
        st = np.zeros((self.G, 16), np.int8)
        rd = np.zeros((self.G, 16), np.uint16)
        fin = np.zeros((self.G, 16, 160), np.uint8)
        self._chk(self.L.azr_arena_log(self.h, _p(n), _p(st), _p(rd), _p(fin)))
        return n, st, rd, fin

    def synchronize(self):
        self._chk(self.L.azr_device_synchronize(self.h))
