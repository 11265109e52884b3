"""GPU parity of the two-net arena between nets of DIFFERENT depth and arithmetic (azr_arena_set_opponent_net with an opponent handle
whose blocks / net_dtype are not the arena handle's): bit-exact against the oracle's game driver with the two DEVICE nets called back per
evaluation, the counted (no read-back) form against the read-back form, the counted launch of the NET_F32X tower alone, the guards
that stay, and the side-by-side rule of the split-channel tower beside a launch that is not its own kind.

The oracle construction is that of tests/test_gpu_arena.py::test_two_net_arena_bit_exact_with_samples.  It rests on every tower
computing the same bits for a board whatever batch it arrives in: documented for the 16-bit towers (tile shapes),
asserted here for NET_F32X and NET_F32 first, so that a mismatch below points at the arena and not at the net."""
import ctypes as C

import numpy as np
import pytest

import azr_testlib as T
from gpu_common import pkg

pytestmark = pytest.mark.gpu
FM = T.data_field_mask()


def run_arena(eng, k0, k1, total, cap, mirror, base):
    eng.arena_start(k0, k1, total, per_slot_cap=cap, mirror=mirror, base_seed=base)
    for _ in range(2000):
        if eng.arena_run(64):
            break
    else:
        raise AssertionError("arena did not finish")
    return eng.arena_results(), eng.arena_log()


def golden_boards(n):
    x = np.load(T.GOLDEN + "/encode.npz")["in88"]
    return x[:: len(x) // n][:n].copy()


def make_eval(eng):
    @T.EVAL_FN
    def f(ctx, in88, pi, v):
        x = np.ctypeslib.as_array(in88, shape=(88,)).copy()[None]
        p, vv = eng.predict(x)
        C.memmove(pi, p.ctypes.data, 43 * 4)
        v[0] = float(vv[0])
    return f


# ---- the premise: a board's outputs do not depend on the batch around it -------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["NET_F32X", "NET_F32"])
def test_a_boards_bits_do_not_depend_on_its_batch(dtype):
    P = pkg()
    B = 2
    x = golden_boards(128)
    eng = P.Engine(128, blocks=B, sims=1, dtype=getattr(P, dtype), node_capacity=64)
    eng.set_weights(T.make_net_flat(B, seed=5, perturb_bn=True))
    pi128, v128 = eng.predict(x)
    assert np.isfinite(pi128).all() and np.isfinite(v128).all()
    for i in (0, 1, 2, 77, 126, 127):        # first / second board of a pair, the last pair
        p1, v1 = eng.predict(x[i:i + 1])
        assert p1.tobytes() == pi128[i:i + 1].tobytes() and v1.tobytes() == v128[i:i + 1].tobytes(), (dtype, i)
    for n in (2, 3):
        for i0 in (0, 1, 125):
            pn, vn = eng.predict(x[i0:i0 + n])
            assert pn.tobytes() == pi128[i0:i0 + n].tobytes() and vn.tobytes() == v128[i0:i0 + n].tobytes(), (dtype, n, i0)
    eng.close()


# ---- 1. mixed arenas against the oracle ----------------------------------------------------------------------------------------------
#            name                  A: dtype, blocks, seed      B: dtype, blocks, seed
PAIRINGS = {
    "bf16_b1-bf16_b2": (("NET_BF16", 1, 31), ("NET_BF16", 2, 32)),
    "f32x_b2-f32x_b1": (("NET_F32X", 2, 33), ("NET_F32X", 1, 34)),
    "bf16-f32x_same_net": (("NET_BF16", 2, 35), ("NET_F32X", 2, 35)),
    "f16-f32": (("NET_F16", 1, 36), ("NET_F32", 1, 37)),
    "f32x_b1-bf16_b2": (("NET_F32X", 1, 38), ("NET_BF16", 2, 39)),
}


def _half_slot(g, G, base):
    return g & 1, base + (g >> 1), G // 2


@pytest.mark.parametrize("mirror", ["sequential", "concurrent"])
@pytest.mark.parametrize("b_first", [False, True])
@pytest.mark.parametrize("threads", [1, 2])
@pytest.mark.parametrize("pairing", sorted(PAIRINGS))
def test_mixed_two_net_arena_bit_exact_with_samples(orc, monkeypatch, pairing, threads, b_first, mirror):
    """statuses, round counts, final states, the six GameResults numbers and every (s, pi, z) record of both players against the
    oracle.  Pairings without a NET_F32 side run in the test build under AZR_ARENA_COUNTED=2, which turns a silent drop to the read-back
    form into AZR_E_STATE: they must run counted.  On the parent of this change every case fails at arena_set_opponent."""
    P = pkg()
    (da, ba, sa), (db, bb, sb) = PAIRINGS[pairing]
    G, per_slot, S, base = 6, 2, 12, 5200
    reads_back = "NET_F32" in (da, db)
    if not reads_back:
        monkeypatch.setenv("AZR_ARENA_COUNTED", "2")
    a = P.Engine(G, blocks=ba, sims=S, dtype=getattr(P, da), threads=threads, max_game_rounds=40, test_hooks=not reads_back)
    b = P.Engine(G, blocks=bb, sims=S, dtype=getattr(P, db), threads=threads, max_game_rounds=40, test_hooks=not reads_back)
    a.set_weights(T.make_net_flat(ba, seed=sa, perturb_bn=True))
    b.set_weights(T.make_net_flat(bb, seed=sb, perturb_bn=True))
    a.arena_set_opponent(b)
    a.arena_collect_samples(True)
    k = (P.PLAYER_ALPHAZERO_B, P.PLAYER_ALPHAZERO) if b_first else (P.PLAYER_ALPHAZERO, P.PLAYER_ALPHAZERO_B)
    mode = P.MIRROR_CONCURRENT if mirror == "concurrent" else P.MIRROR_SEQUENTIAL
    res, (n, st, rd, fin) = run_arena(a, k[0], k[1], 10 ** 6, per_slot, mode, base)
    c = a.counters()
    assert (n == per_slot).all() and c["errors"] == 0 and c["nodes_dropped"] == 0 and c["tower_fallbacks"] == 0
    recs = a.drain()

    ea, eb = make_eval(a), make_eval(b)
    cfg = T.default_settings(mcts_simulations=S, mcts_threads=threads, max_game_rounds=40)
    tot = np.zeros(6, np.int64)
    blob = recs.tobytes()
    nrec = 0
    for g in range(G):
        if mirror == "concurrent":
            half, q0, stride = _half_slot(g, G, base)
            r6, ost, ord_, ofin, orec = T.orc_play_half_games(k[0], k[1], per_slot, half, q0, stride, cfg, ea, eb)
        else:
            r6, ost, ord_, ofin, orec = T.orc_play_games2(k[0], k[1], per_slot, True, base + g, cfg, ea, eb)
        assert (st[g, :per_slot] == ost).all(), (g, st[g], ost)
        assert (rd[g, :per_slot] == ord_).all(), g
        assert (fin[g, :per_slot][:, FM] == ofin[:, FM]).all(), g
        tot += np.array(r6)
        for gi, game in enumerate(orec):   # a finished game's records are flushed contiguously, z filled in
            assert len(game) > 0 and game.tobytes() in blob, (g, gi)
            nrec += len(game)
    assert nrec == len(recs)
    assert [res["count"], res["draw"], res["win"][0], res["win_and_started"][0], res["win"][1], res["win_and_started"][1]] == list(tot)
    a.arena_set_opponent(None)
    a.close(); b.close()


def test_an_arena_with_an_f32_side_reads_back(monkeypatch):
    """NET_F32 has no counted launch: under AZR_ARENA_COUNTED=2 its arena must say that it reads back (and play as usual without)"""
    P = pkg()
    monkeypatch.setenv("AZR_ARENA_COUNTED", "2")
    a = P.Engine(6, blocks=1, sims=4, dtype=P.NET_F16, threads=2, max_game_rounds=40, test_hooks=True)
    b = P.Engine(6, blocks=1, sims=4, dtype=P.NET_F32, threads=2, max_game_rounds=40, test_hooks=True)
    a.init_random(1); b.init_random(2)
    a.arena_set_opponent(b)
    a.arena_start(P.PLAYER_ALPHAZERO, P.PLAYER_ALPHAZERO_B, 4, 0, P.MIRROR_SEQUENTIAL, 1)
    with pytest.raises(P.binding.AzrError) as e:
        a.arena_run(8)
    assert e.value.code == 7 and "reads back" in str(e.value)          # AZR_E_STATE
    monkeypatch.delenv("AZR_ARENA_COUNTED")
    res, _ = run_arena(a, P.PLAYER_ALPHAZERO, P.PLAYER_ALPHAZERO_B, 4, 0, P.MIRROR_SEQUENTIAL, 1)
    assert res["count"] == 4 and a.counters()["errors"] == 0
    a.arena_set_opponent(None)
    a.close(); b.close()


# ---- 2. counted equals read-back; 5. the side-by-side rule beside a launch of another kind ---------------------------------------------
def _big_arena(P, monkeypatch, env, da, db, G, games):
    """one arena of G slots x T = 2 in the test build under the environment `env`; everything a caller can see of it"""
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    S, B, base = 6, 1, 9100
    a = P.Engine(G, blocks=B, sims=S, dtype=getattr(P, da), threads=2, max_game_rounds=30, test_hooks=True)
    b = P.Engine(G, blocks=B, sims=S, dtype=getattr(P, db), threads=2, max_game_rounds=30, test_hooks=True)
    a.set_weights(T.make_net_flat(B, seed=41, perturb_bn=True))
    b.set_weights(T.make_net_flat(B, seed=42, perturb_bn=True))
    a.arena_set_opponent(b)
    a.arena_collect_samples(True)
    res, (n, st, rd, fin) = run_arena(a, P.PLAYER_ALPHAZERO, P.PLAYER_ALPHAZERO_B, games, 0, P.MIRROR_SEQUENTIAL, base)
    c = a.counters()
    assert c["errors"] == 0 and c["nodes_dropped"] == 0 and c["tower_fallbacks"] == 0 and c["records_dropped"] == 0
    recs = a.drain()
    a.arena_set_opponent(None)
    a.close(); b.close()
    for k_ in env:
        monkeypatch.delenv(k_)
    assert res["count"] == games
    return res, n.copy(), st.copy(), rd.copy(), fin.copy(), b"".join(sorted(r.tobytes() for r in recs))


def _same(x, y):
    assert x[0] == y[0]
    for p, q in zip(x[1:5], y[1:5]):
        assert (p == q).all()
    assert len(x[5]) > 0 and x[5] == y[5]


@pytest.mark.parametrize("da,db", [("NET_BF16", "NET_F32X"), ("NET_F32X", "NET_F32X")])
def test_mixed_passes_without_a_read_back_equal_the_read_back_form(monkeypatch, da, db):
    """128 slots x T = 2 = 256 leaf slots, the bound of the counted form: the default run (under AZR_ARENA_COUNTED=2, so it IS the
    counted form) and the run with AZR_ARENA_COUNTED=0 give the same results, logs and sorted record bytes"""
    P = pkg()
    counted = _big_arena(P, monkeypatch, {"AZR_ARENA_COUNTED": "2"}, da, db, 128, 256)
    read_back = _big_arena(P, monkeypatch, {"AZR_ARENA_COUNTED": "0"}, da, db, 128, 256)
    _same(counted, read_back)


@pytest.mark.parametrize("G", [32, 128])
def test_side_by_side_rule_beside_an_f32x_launch_changes_no_result(monkeypatch, G):
    """k_tower_sc told 1 workgroup per board pair for the launch beside it (AZR_ARENA_BESIDE_WGPP=1: what k_tower_fx<2> really spends)
    keeps its four-workgroups-per-pair form while 4 * pairs_n + 1 * pairs_m <= 256 and hands the batch to the one-board-per-workgroup
    launch above that.  With 32 slots (at most 64 leaves in all: 4 * 32 + 32 <= 256) it always keeps it; with 128 slots the passes (up
    to 256 leaves of one net in the opening, then about half and half: 4 * 32 + 32 ... 4 * 64 + 64) cross the bound both ways.  The
    rule may change a time, never a result: the same arena with the other launch charged with 256 per pair (every pass with a leaf on
    both sides hands over), as the product's plan charges it, and in the read-back form (no rule at all: the host sizes each launch)
    must agree bit for bit, and no launch may count as given up (asserted in _big_arena)."""
    P = pkg()
    games = 2 * G
    rule = _big_arena(P, monkeypatch, {"AZR_ARENA_COUNTED": "2", "AZR_ARENA_BESIDE_WGPP": "1"}, "NET_BF16", "NET_F32X", G, games)
    always_over = _big_arena(P, monkeypatch, {"AZR_ARENA_COUNTED": "2", "AZR_ARENA_BESIDE_WGPP": "256"}, "NET_BF16", "NET_F32X", G, games)
    plan = _big_arena(P, monkeypatch, {"AZR_ARENA_COUNTED": "2"}, "NET_BF16", "NET_F32X", G, games)
    read_back = _big_arena(P, monkeypatch, {"AZR_ARENA_COUNTED": "0"}, "NET_BF16", "NET_F32X", G, games)
    _same(rule, always_over)
    _same(rule, plan)
    _same(rule, read_back)
    # the opponent side too: the F32X handle runs the arena, the split-channel tower is the launch on the other stream
    rule_b = _big_arena(P, monkeypatch, {"AZR_ARENA_COUNTED": "2", "AZR_ARENA_BESIDE_WGPP": "1"}, "NET_F32X", "NET_BF16", G, games)
    read_back_b = _big_arena(P, monkeypatch, {"AZR_ARENA_COUNTED": "0"}, "NET_F32X", "NET_BF16", G, games)
    _same(rule_b, read_back_b)


# ---- 3. the counted launch of k_tower_fx alone ------------------------------------------------------------------------------------------
def test_f32x_counted_launch_equals_the_plain_one_and_writes_nothing_past_the_count(monkeypatch):
    """AZR_PREDICT_COUNTED=N (test build) sends predict through net_forward_counted: the batch size, capped at N, in a device word, the
    grid sized for the handle's 128 leaf slots.  Same bits as the plain launch for n = 1, 2, 3, 127, 128; and a call whose count is
    below its batch returns, from the count on, what the call before left in the device outputs — workgroups past the count (and the
    masked second board of the last one) wrote nothing."""
    P = pkg()
    B = 2
    x = golden_boards(128)
    eng = P.Engine(128, blocks=B, sims=1, dtype=P.NET_F32X, node_capacity=64, test_hooks=True)
    eng.set_weights(T.make_net_flat(B, seed=6, perturb_bn=True))
    plain_pi, plain_v = eng.predict(x)
    for n in (1, 2, 3, 127, 128):
        monkeypatch.setenv("AZR_PREDICT_COUNTED", "1000")
        pi, v = eng.predict(x[:n])
        monkeypatch.delenv("AZR_PREDICT_COUNTED")
        assert pi.tobytes() == plain_pi[:n].tobytes() and v.tobytes() == plain_v[:n].tobytes(), n
    y = x[::-1].copy()
    want_pi, want_v = eng.predict(y)
    assert want_pi[3:].tobytes() != plain_pi[3:].tobytes()
    for n in (3, 1, 64):
        monkeypatch.setenv("AZR_PREDICT_COUNTED", "1000")
        eng.predict(x)                                      # every slot's device output = x's
        monkeypatch.setenv("AZR_PREDICT_COUNTED", str(n))
        pi, v = eng.predict(y)                              # 128 boards staged, the device word says n
        monkeypatch.delenv("AZR_PREDICT_COUNTED")
        assert pi[:n].tobytes() == want_pi[:n].tobytes() and v[:n].tobytes() == want_v[:n].tobytes(), n
        assert pi[n:].tobytes() == plain_pi[n:].tobytes() and v[n:].tobytes() == plain_v[n:].tobytes(), n
    eng.close()


# ---- 4. the guards that stay ----------------------------------------------------------------------------------------------------------
def test_guards_kept():
    P = pkg()
    a = P.Engine(8, blocks=1, sims=4, dtype=P.NET_BF16, threads=2, max_game_rounds=30)
    few = P.Engine(8, blocks=2, sims=4, dtype=P.NET_F32X, threads=1)       # 8 leaf slots against a's 16
    a.init_random(1); few.init_random(2)
    with pytest.raises(P.binding.AzrError) as e:
        a.arena_set_opponent(few)
    assert e.value.code == 1 and "leaf slots" in str(e.value) and "shape" not in str(e.value)   # AZR_E_INVALID_ARGUMENT
    few.arena_set_opponent(a)            # the other way round there are enough
    few.arena_set_opponent(None)
    a.arena_set_opponent(None)
    with pytest.raises(P.binding.AzrError) as e:
        a.arena_start(P.PLAYER_ALPHAZERO, P.PLAYER_ALPHAZERO_B, 4, 0, P.MIRROR_SEQUENTIAL, 1)
    assert e.value.code == 7                                                                    # AZR_E_STATE
    a.arena_set_opponent(a)              # a handle as its own opponent: one net, two trees
    res, _ = run_arena(a, P.PLAYER_ALPHAZERO, P.PLAYER_ALPHAZERO_B, 8, 0, P.MIRROR_CONCURRENT, 3)
    assert res["count"] == 8 and a.counters()["errors"] == 0
    a.arena_set_opponent(None)
    a.close(); few.close()
