"""The rules layer off its default settings (TEST INFRASTRUCTURE): the settings the lock-step, move-sweep, arena and search tests
run at, the oracle's random-policy games under them, and a census of the situations those games reach.

The census is plain Python over the oracle's states and the neighbour lists of tests/golden/tables.npz.  It restates the branch
conditions of UtilityNN::makeMove (alphazero_moves.cpp:104-231) and nothing of their results: it says which branch an input takes, so
that a test can require its inputs to take every one of them."""
import ctypes as C
import os

import numpy as np

import azr_testlib as T

ARMY_MAX, SKIP = 32, 42
PH_REINFORCEMENT, PH_ATTACK, PH_MOBILIZATION, PH_FORTIFY = 2, 3, 4, 5
FIVE = dict(allow_yield=0, limit_reinforcement=0, limit_attack=1, max_game_rounds=120, min_unit_move=2)
LONG = dict(allow_yield=0, max_game_rounds=150)
# the lock-step settings: 32 games each, seeds 3000 upwards ...
SETTINGS = [dict(limit_reinforcement=0), dict(limit_attack=1), dict(min_unit_move=1), dict(min_unit_move=5), LONG, FIVE]
SEED0, GAMES = 3000, 32
# ... and, where those 32 games reach a situation fewer than CENSUS_MIN times, the next seeds whose game (in the oracle, under that
# setting) ends in it.  A drawn game also ends at the round limit, so the draw seeds serve both.
EXTRA_SEEDS = {
    # draws (the 32 games hold 1)
    "limit_reinforcement=0": [3073, 3102, 3149, 3173, 3219, 3267, 3273, 3414, 3417, 3424],
    # forced attacks end a game long before round 58: 11 round-limit ends in seeds 3032..7589, 11 draws in 3032..73965 (of 32: none)
    "limit_attack=1": [3370, 3874, 3902, 5468, 5708, 5809, 6182, 6651, 6656, 7290, 7589,
                       22124, 22831, 23317, 24742, 28038, 32198, 35538, 60976, 63513, 65754, 73965],
    # draws (2); with them the round limit, which ends 8 of the 32
    "min_unit_move=1": [3053, 3127, 3171, 3209, 3343, 3368, 3464, 3631, 3853],
    # draws (0); the round limit ends 9 of the 32
    "min_unit_move=5": [3170, 3190, 3242, 3251, 3334, 3570, 3669, 3697, 3701, 3881, 3921],
    # draws at round 151 (0); the round limit ends 7 of the 32
    "allow_yield=0,max_game_rounds=150": [3479, 4565, 5558, 7730, 8695, 9696, 10635, 11021, 11703, 12829, 12897],
    # draws at round 121 (0)
    "allow_yield=0,limit_reinforcement=0,limit_attack=1,max_game_rounds=120,min_unit_move=2":
        [3251, 3489, 3738, 4199, 4256, 4314, 4339, 4507, 4841, 5390, 5519],
}

SITUATIONS = ("reinforce_clamped", "reinforce_skip_only", "fortify_target_full", "fortify_clamped", "fortify_source_tie",
              "fortify_source_unique", "attack_source_tie", "attack_source_unique", "mobilize_half", "mobilize_min_unit",
              "mobilize_all", "card_set_7_up", "round_limit_end", "draw")
# Saturation (an army of ARMY_MAX) and the seventh card set need a long game.  With ALLOW_YIELD a game ends once a player owns 30
# lands, at round 58 at the latest: the default test's 256 such games reach a full fortify target 5 times.  So these five are required
# of the two settings that play 120 and 150 rounds without yield, and of no other.
LONG_GAME_ONLY = ("reinforce_clamped", "reinforce_skip_only", "fortify_target_full", "fortify_clamped", "card_set_7_up")
CENSUS_MIN = 10


def setting_id(kw):
    return ",".join(f"{k}={v}" for k, v in kw.items())


def seeds(kw):
    return np.array(list(range(SEED0, SEED0 + GAMES)) + EXTRA_SEEDS.get(setting_id(kw), []), np.uint32)


def required(kw):
    """the situations a setting's games must reach CENSUS_MIN times: every one that can occur under it"""
    need = set(SITUATIONS)
    if kw.get("allow_yield", 1) or kw.get("max_game_rounds", 58) < 100:
        need -= set(LONG_GAME_ONLY)
    if kw.get("min_unit_move", 3) == 1:
        need.discard("mobilize_all")   # value < 1 never holds: a mobilisation's source has at least 2 armies
    return need


_nb = None


def neighbours():
    global _nb
    if _nb is None:
        t = np.load(os.path.join(T.GOLDEN, "tables.npz"))
        _nb = [[int(x) for x in t["neighbours"][l][:int(t["neighbour_count"][l])]] for l in range(42)]
    return _nb


def _component(owned, start):
    nb, seen, todo = neighbours(), {start}, [start]
    while todo:
        for n in nb[todo.pop()]:
            if n in owned and n not in seen:
                seen.add(n)
                todo.append(n)
    return seen


def _tied(values):
    """(tie, unique) of a list of candidate values: how many hold the maximum"""
    if not values:
        return False, False
    k = values.count(max(values))
    return k > 1, k == 1


def classify(s, mask, mv, kw):
    """the situations of playing move mv (legal mask `mask`) in the OrcState s under the settings kw"""
    out = []
    nb = neighbours()
    p = s.cur
    army, owner = list(s.army), list(s.owner)
    mum = kw.get("min_unit_move", 3)
    if s.phase == PH_REINFORCEMENT:
        reinf = s.reinf
        if s.ps[p].cards >= 3:   # playCards runs first
            sets = s.card_sets + 1
            if sets >= 7:
                out.append("card_set_7_up")
            reinf += {1: 4, 2: 6, 3: 8, 4: 10, 5: 12, 6: 15}.get(sets, 15 + (sets - 6) * 5)
        if mv == SKIP:
            if mask == 1 << SKIP:
                out.append("reinforce_skip_only")
        else:
            want = reinf // 2
            if want < mum:
                want = min(mum, reinf)
            if ARMY_MAX - army[mv] < want:
                out.append("reinforce_clamped")
    elif s.phase == PH_ATTACK and mv != SKIP:
        tie, unique = _tied([army[n] - 1 for n in nb[mv] if owner[n] == p and army[n] > 1])
        out += ["attack_source_tie"] * tie + ["attack_source_unique"] * unique
    elif s.phase == PH_MOBILIZATION and mv == s.mob_to:
        value = army[s.mob_from] - 1
        out.append("mobilize_half" if value // 2 >= mum else "mobilize_min_unit" if mum <= value else "mobilize_all")
    elif s.phase == PH_FORTIFY and mv != SKIP and owner[mv] == p:
        if army[mv] == ARMY_MAX:
            out.append("fortify_target_full")
        else:
            owned = {l for l in range(42) if owner[l] == p}
            cand = [l for l in _component(owned, mv) if l != mv and army[l] > 1]
            inner = [army[l] - 1 for l in cand if all(n in owned for n in nb[l])]
            border = [army[l] - 1 for l in cand if not all(n in owned for n in nb[l])]
            cls = inner or border   # lands with every neighbour owned come first
            tie, unique = _tied(cls)
            out += ["fortify_source_tie"] * tie + ["fortify_source_unique"] * unique
            if cls and ARMY_MAX - army[mv] < max(cls):
                out.append("fortify_clamped")
    return out


def classify_end(final, status, kw):
    """the situations of a finished game: OrcState `final`, its status"""
    out = []
    if status == -2:
        out.append("draw")
    n0, n1 = (sum(1 for l in range(42) if final.owner[l] == q) for q in (0, 1))
    by_yield = kw.get("allow_yield", 1) and max(n0, n1) >= 30
    if n0 and n1 and not by_yield and final.round > kw.get("max_game_rounds", 58):
        out.append("round_limit_end")
    return out


_games = {}


def oracle_games(kw):
    """the random-policy games of a setting (the golden generator's policy: moves by randomMask from the stream the dice use), once
    per setting and shared: list of dict(states, masks, moves, status, final) as azr_testlib.orc_random_game; read only"""
    key = setting_id(kw)
    if key not in _games:
        cfg = T.default_settings(**kw)
        _games[key] = [T.orc_random_game(int(seed), cap=65536, cfg=cfg) for seed in seeds(kw)]
    return _games[key]


_census = {}


def census(kw):
    """how often the setting's games reach each situation"""
    key = setting_id(kw)
    if key not in _census:
        L = T.oracle()
        count = dict.fromkeys(SITUATIONS, 0)
        s = T.OrcState()
        for g in oracle_games(kw):
            for st, mask, mv in zip(g["states"], g["masks"], g["moves"]):
                L.orc_state_unpack(C.byref(s), T.ptr(st))
                for k in classify(s, int(mask), int(mv), kw):
                    count[k] += 1
            L.orc_state_unpack(C.byref(s), T.ptr(g["final"]))
            for k in classify_end(s, g["status"], kw):
                count[k] += 1
        _census[key] = count
    return _census[key]


def sweep_states(n=102):
    """about 100 states of all six phases from the long games of LONG and FIVE, a third of them saturated (a full land of the player
    to move) where the games hold that many; the same list for every caller"""
    picked = []
    for kw in (LONG, FIVE):
        pool = np.concatenate([g["states"] for g in oracle_games(kw)])
        phase, cur = pool[:, 149], pool[:, 146]
        lands = pool[:, 0:42]   # army | owner << 6
        full = (lands == (ARMY_MAX | (cur[:, None] << 6))).any(1)
        for ph in range(6):
            for sat in (True, False):
                idx = np.nonzero((phase == ph) & (full == sat))[0]
                want = n // 24 + (1 if sat else 4)
                picked += [pool[i] for i in idx[::max(1, len(idx) // want)][:want]]
    return np.array(picked)[:n] if len(picked) > n else np.array(picked)


def search_roots(n=48):
    """n states of FIVE's games for the search tests: reinforcement, attack, mobilisation and fortify in equal parts, half of each
    with a full land of the player to move"""
    pool = np.concatenate([g["states"] for g in oracle_games(FIVE)])
    phase, cur = pool[:, 149], pool[:, 146]
    full = (pool[:, 0:42] == (ARMY_MAX | (cur[:, None] << 6))).any(1)
    picked = []
    for ph in (PH_REINFORCEMENT, PH_ATTACK, PH_MOBILIZATION, PH_FORTIFY):
        for sat in (True, False):
            idx = np.nonzero((phase == ph) & (full == sat))[0]
            want = n // 8
            picked += [pool[i] for i in idx[::len(idx) // want][:want]]
    return np.array(picked)
