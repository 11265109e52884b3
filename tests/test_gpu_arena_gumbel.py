"""GPU: the Gumbel search with sequential halving per AlphaZero side of an arena (azr_arena_set_gumbel).  The oracle has no such search:
the proof is the host-stepped retrace of tests/arena_retrace.py — one pair of games per slot, NET_F32 nets of 1-2 blocks; 4 slots and 12
rounds (SHORT: the setup phase) where that is enough, 2 slots and 28 rounds (LONG: past the setup phase, into the turns that attack)
for case 2.

  1. the harness   both sides PUCT at budgets 12 and 8: the retrace gives the arena's records, log, six result numbers and simulation
                   count bit for bit at T = 1 and 2 (this case needs nothing of the feature: it is what lets the others mean something)
  2. both Gumbel   A: m = 4, 12 simulations, PUCT below the root; B: m = 3, 9 simulations at T = 2 (so 8), the improved-policy selection
                   below the root; one net on both sides, and nets of 1 and 2 blocks with the kinds in both orders.  Not vacuous: some
                   decision starts from a root with visits (N0), some has more legal moves than m, some fewer
  3. mixed         A PUCT against B Gumbel and the reverse: the PUCT side inside the new step
  4. collecting    one net against Script and Random with the Gumbel side collecting: pi sums to 1, is no visit distribution, two runs agree
                   (NET_F32 arenas read back after every pass: a bf16 arena under AZR_ARENA_COUNTED=2 runs the step in the counted form)
  5. off           m = 0 on both sides is the engine that never called the setter; a setting for a player the arena does not have too
  6. guards        refusals, AZR_E_STATE during an arena, scripted collection, the reset, self-play untouched

Every case but 1 fails without azr_arena_set_gumbel, at the missing symbol."""
import numpy as np
import pytest

import arena_retrace as R
from arena_retrace import Side
from gpu_common import pkg

pytestmark = pytest.mark.gpu
BASE = 8100
_cache = {}


def kinds_of(P, b_first):
    return (P.PLAYER_ALPHAZERO_B, P.PLAYER_ALPHAZERO) if b_first else (P.PLAYER_ALPHAZERO, P.PLAYER_ALPHAZERO_B)


def retraced(P, a, b, threads, b_first, shape, base=BASE):
    """the retrace of one pairing, computed once per process; callers must not write into it"""
    key = (a, b, threads, b_first, shape, base)
    if key not in _cache:
        _cache[key] = R.retrace(P, {P.PLAYER_ALPHAZERO: a, P.PLAYER_ALPHAZERO_B: b}, threads, kinds_of(P, b_first), base, shape)
    return _cache[key]


def arena_against_retrace(a, b, threads, shape, b_first=False, one_net=False, base=BASE):
    P = pkg()
    eng, opp = R.arena_engines(P, a, b, threads, shape, one_net)
    R.configure(P, eng, a, b)
    got = R.play(eng, kinds_of(P, b_first), base)
    R.close(eng, opp)
    games = retraced(P, a, b, threads, b_first, shape, base)
    print("arena: results", got[0], "status", got[1], "rounds", got[2], "simulations", got[5], "records", len(got[4]) // 265,
          "| retrace: decisions", [len(x.decisions) for x in games])
    R.assert_same(got, R.expected(games))
    return games


# ---- 1. the harness -------------------------------------------------------------------------------------------------------------------
PUCT_A, PUCT_B = Side(12, 1.3), Side(8, 2.0, seed=32)


@pytest.mark.parametrize("threads", [1, 2])
def test_the_retrace_gives_a_puct_arena_bit_for_bit(threads):
    """no setter of the feature is called on the arena handle: R.configure is left out on purpose"""
    P = pkg()
    eng, opp = R.arena_engines(P, PUCT_A, PUCT_B, threads, R.SHORT)
    eng.arena_set_opponent_search(PUCT_B.sims, PUCT_B.hp)
    got = R.play(eng, kinds_of(P, False), BASE)
    R.close(eng, opp)
    R.assert_same(got, R.expected(retraced(P, PUCT_A, PUCT_B, threads, False, R.SHORT)))


# ---- 2. both sides Gumbel -------------------------------------------------------------------------------------------------------------
GUM_A, GUM_B = Side(12, 1.3, m=4, tree=0), Side(9, 2.0, m=3, tree=1, seed=32)


@pytest.mark.parametrize("one_net,blocks_b,b_first", [(True, 1, False), (False, 2, False), (False, 2, True)])
def test_both_sides_gumbel_bit_for_bit(one_net, blocks_b, b_first):
    b = GUM_B._replace(seed=GUM_A.seed) if one_net else GUM_B._replace(blocks=blocks_b)
    games = arena_against_retrace(GUM_A, b, 2, R.LONG, b_first, one_net)
    dec = [d for x in games for d in x.decisions]
    n0, more, fewer = sum(d[0] > 0 for d in dec), sum(d[1] > d[2] for d in dec), sum(d[1] < d[2] for d in dec)
    print("decisions", len(dec), "from a root with visits", n0, "more legal moves than m", more, "fewer", fewer)
    assert n0 > 0 and more > 0 and fewer > 0          # N0 counted, m_eff = m and m_eff = the legal moves all occur


# ---- 3. mixed -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b,threads", [(PUCT_A, GUM_B, 2), (GUM_A, PUCT_B, 1)])
def test_a_puct_side_beside_a_gumbel_side_bit_for_bit(a, b, threads):
    games = arena_against_retrace(a, b, threads, R.SHORT)
    assert {d[2] for x in games for d in x.decisions} == {a.m, b.m}   # both sides decided


# ---- 4. one net against Script and Random, the Gumbel side collecting -----------------------------------------------------------------
@pytest.mark.parametrize("other,az_first", [("script", True), ("random", False)])
def test_the_gumbel_side_collects_its_improved_policy(other, az_first):
    P = pkg()
    n = 12
    k = P.PLAYER_SCRIPT if other == "script" else P.PLAYER_RANDOM
    kinds = (P.PLAYER_ALPHAZERO, k) if az_first else (k, P.PLAYER_ALPHAZERO)
    eng = R.engine(P, Side(n), 2, 4, R.LONG.rounds)
    eng.arena_set_gumbel(P.PLAYER_ALPHAZERO, 4, R.CV, R.CS, 1)
    one = R.play(eng, kinds, BASE)                      # finishes, errors = nodes_dropped = records_dropped = 0
    two = R.play(eng, kinds, BASE)
    eng.close()
    R.assert_same(one, two)
    recs = np.frombuffer(one[4], np.uint8).reshape(-1, 265)
    assert len(recs) > 0
    pi = recs[:, 93:265].copy().view(np.float32).astype(np.float64)
    assert np.abs(pi.sum(1) - 1).max() <= 43 * 2.0 ** -24
    assert (np.abs(pi * n - np.rint(pi * n)) > 1e-3).any()   # no visit distribution: not all multiples of 1 / n


def test_the_arena_form_without_a_read_back_runs_the_gumbel_step(monkeypatch):
    """The retraces run on NET_F32, whose arenas read the leaf counts back after every pass.  bf16 nets take the counted form, where the
    step alternates between two count rows: in the test build under AZR_ARENA_COUNTED=2 (a drop to the read-back form is AZR_E_STATE)
    a Gumbel arena of concurrent mirrored pairs finishes clean, two runs give the same bytes, and PUCT on both sides gives others"""
    import azr_testlib as T
    P = pkg()
    monkeypatch.setenv("AZR_ARENA_COUNTED", "2")
    kw = dict(sims=12, dtype=P.NET_BF16, threads=2, max_game_rounds=R.LONG.rounds, test_hooks=True)
    a, b = P.Engine(6, blocks=1, **kw), P.Engine(6, blocks=2, **kw)
    a.set_weights(T.make_net_flat(1, seed=31, perturb_bn=True)); b.set_weights(T.make_net_flat(2, seed=32, perturb_bn=True))
    a.arena_set_opponent(b)
    a.arena_collect_samples(True)

    def run():
        a.arena_start(P.PLAYER_ALPHAZERO, P.PLAYER_ALPHAZERO_B, 10 ** 6, per_slot_cap=2, mirror=P.MIRROR_CONCURRENT, base_seed=BASE)
        for _ in range(2000):
            if a.arena_run(64):
                break
        else:
            raise AssertionError("arena did not finish")
        c, (n, st, rd, fin) = a.counters(), a.arena_log()
        assert (n == 2).all() and c["errors"] == 0 and c["nodes_dropped"] == 0 and c["records_dropped"] == 0, (n, c)
        return a.arena_results(), st[:, :2].tobytes(), rd[:, :2].tobytes(), b"".join(sorted(x.tobytes() for x in a.drain())), c["simulations"]

    R.configure(P, a, GUM_A, GUM_B)
    one, two = run(), run()
    assert one == two and len(one[3]) > 0
    R.configure(P, a, PUCT_A, PUCT_B)
    assert run()[3] != one[3]
    a.arena_set_opponent(None)
    a.close(); b.close()


# ---- 5. off ---------------------------------------------------------------------------------------------------------------------------
def test_off_is_the_engine_that_never_called_the_setter():
    P = pkg()
    eng, opp = R.arena_engines(P, PUCT_A, PUCT_B, 2, R.SHORT)
    eng.arena_set_opponent_search(PUCT_B.sims, PUCT_B.hp)
    never = R.play(eng, kinds_of(P, False), BASE)
    R.configure(P, eng, PUCT_A, PUCT_B)                 # m = 0 on both sides
    R.assert_same(R.play(eng, kinds_of(P, False), BASE), never)
    R.configure(P, eng, GUM_A, PUCT_B)                  # ... and a Gumbel side does change the games
    assert R.play(eng, kinds_of(P, False), BASE)[4] != never[4]
    R.close(eng, opp)


def test_a_setting_for_a_player_the_arena_does_not_have_changes_nothing():
    P = pkg()
    eng = R.engine(P, Side(12), 2, 4, R.LONG.rounds)
    kinds = (P.PLAYER_ALPHAZERO, P.PLAYER_SCRIPT)
    before = R.play(eng, kinds, BASE)
    eng.arena_set_opponent(eng)
    eng.arena_set_gumbel(P.PLAYER_ALPHAZERO_B, 4, R.CV, R.CS, 1)
    R.assert_same(R.play(eng, kinds, BASE), before)
    eng.arena_set_opponent(None)
    eng.close()


# ---- 6. guards ------------------------------------------------------------------------------------------------------------------------
def refused(P, call, code, *words):
    with pytest.raises(P.binding.AzrError) as e:
        call()
    assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)


def test_guards():
    P = pkg()
    A, B = P.PLAYER_ALPHAZERO, P.PLAYER_ALPHAZERO_B
    eng, opp = R.arena_engines(P, GUM_A, GUM_B, 2, R.Shape(2, 12))
    R.configure(P, eng, GUM_A, GUM_B)
    kinds = kinds_of(P, False)
    both = R.play(eng, kinds, BASE)
    nan = float("nan")
    for call, word in ((lambda: eng.arena_set_gumbel(P.PLAYER_SCRIPT, 4), "player"), (lambda: eng.arena_set_gumbel(7, 4), "player"),
                       (lambda: eng.arena_set_gumbel(A, 44), "m = 44"), (lambda: eng.arena_set_gumbel(A, -1), "m = -1"),
                       (lambda: eng.arena_set_gumbel(A, 4, nan, 0.5), "finite"), (lambda: eng.arena_set_gumbel(B, 4, 50.0, float("inf")), "finite"),
                       (lambda: eng.arena_set_gumbel(A, 4, 50.0, 0.0), "c_scale"), (lambda: eng.arena_set_gumbel(A, 4, -1.0, 0.5), "c_visit"),
                       (lambda: eng.arena_set_gumbel(A, 4, 50.0, 0.5, 2), "tree"), (lambda: eng.arena_set_gumbel(B, 0, 50.0, 0.5, 1), "tree")):
        refused(P, call, 1, "azr_arena_set_gumbel", word)                       # AZR_E_INVALID_ARGUMENT, the handle as it was
    R.assert_same(R.play(eng, kinds, BASE), both)                               # ... and the setting holds over arena_start calls
    assert eng.L.azr_arena_set_gumbel(None, A, 4, 50.0, 0.5, 0) == 3            # AZR_E_BAD_HANDLE
    # between azr_arena_start and the finish
    eng.arena_start(kinds[0], kinds[1], 10 ** 6, per_slot_cap=1, mirror=P.MIRROR_OFF, base_seed=BASE)
    refused(P, lambda: eng.arena_set_gumbel(A, 0), 7, "an arena is running")    # AZR_E_STATE
    assert not eng.arena_run(1)
    refused(P, lambda: eng.arena_set_gumbel(B, 0), 7, "an arena is running")
    for _ in range(2000):
        if eng.arena_run(64):
            break
    eng.discard_samples()
    eng.arena_set_gumbel(A, 0)                                                   # finished: accepted
    a_off = R.play(eng, kinds, BASE)
    assert a_off[4] != both[4]
    # scripted collection with a Gumbel side: refused at the start, the handle usable afterwards
    eng.arena_set_gumbel(A, 4, R.CV, R.CS, 0)
    eng.arena_collect_scripted_samples(True)
    refused(P, lambda: eng.arena_start(A, P.PLAYER_SCRIPT, 4, per_slot_cap=1, mirror=P.MIRROR_OFF, base_seed=BASE), 1, "azr_arena_start", "scripted")
    eng.arena_collect_scripted_samples(False)
    R.assert_same(R.play(eng, kinds, BASE), both)
    # azr_arena_set_opponent_net(h, NULL) puts player B back to PUCT (and to the handle's budget: set again)
    eng.arena_set_opponent(None)
    eng.arena_set_opponent(opp)
    eng.arena_set_opponent_search(GUM_B.sims, GUM_B.hp)
    b_off = R.play(eng, kinds, BASE)
    assert b_off[4] not in (both[4], a_off[4])
    eng.arena_set_gumbel(B, GUM_B.m, R.CV, R.CS, GUM_B.tree)
    R.assert_same(R.play(eng, kinds, BASE), both)
    R.close(eng, opp)


def test_self_play_is_the_same_before_and_after_a_gumbel_arena():
    P = pkg()
    eng, opp = R.arena_engines(P, GUM_A, GUM_B, 2, R.SHORT, one_net=True)

    def quota():
        eng.selfplay_start_games(77, 3)
        recs = []
        for _ in range(4000):
            eng.selfplay_run(64)
            recs.append(eng.drain())
            c = eng.counters()
            if c["games_finished"] + c["errors"] >= 3:
                break
        assert c["games_finished"] == 3 and c["errors"] == 0 and c["records_dropped"] == 0, c
        return b"".join(sorted(r.tobytes() for r in np.concatenate(recs))), c["simulations"], c["decisions"]

    before = quota()
    R.configure(P, eng, GUM_A, GUM_B._replace(seed=GUM_A.seed))
    assert len(R.play(eng, kinds_of(P, False), BASE)[4]) > 0
    assert quota() == before and len(before[0]) > 0
    R.close(eng, opp)
