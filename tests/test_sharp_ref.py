"""CPU: the sharp stub net (oracle/azr_oracle.c orc_sharp_eval) is what its header says, the oracle's own search under it lies in
the regime the sharp GPU tests are about, and the game-level restatements the device tests rest on (tests/playout_cap_ref.py,
tests/arena_budget_ref.py) still equal the oracle's own games under it with their option neutral.  The row-level restatements
(forced_playouts_ref, value_mix_ref, surprise_ref) run on the roots of that search: neutral they change nothing, on they stay
finite — rows with zero and denormal priors, one move holding every visit, Q of exactly +-1.  The same restatements, and those of
the Gumbel search, its tree selection and resignation, then run on the oracle's own games from selfplay_retrace.late_positions():
neutral, each gives the oracle's game back; on, each gives a policy over the legal moves and a legal move."""
import ctypes as C

import numpy as np
import pytest

import arena_budget_ref as AB
import azr_testlib as T
import forced_playouts_ref as FP
import gumbel_ref as GU
import gumbel_tree_ref as GT
import playout_cap_ref as PC
import resign_ref as RS
import selfplay_retrace as SR
import surprise_ref as SU
import value_mix_ref as VM

f32 = np.float32
M64 = (1 << 64) - 1


def _splitmix64(s):
    s = (s + 0x9E3779B97F4A7C15) & M64
    z = s
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return s, z ^ (z >> 31)


def _draw(x):
    """(mode, a, b, vm) of board x [88]: FNV-1a of the bytes, one splitmix64 step"""
    h = 0xcbf29ce484222325
    for byte in x.tolist():
        h = ((h ^ byte) * 0x100000001b3) & M64
    _, r = _splitmix64(h)
    return r % 8, (r >> 8) % 43, (r >> 16) % 43, (r >> 24) % 6


def _stub(name, x):
    pi, v = np.zeros(43, f32), C.c_float(0)
    xx = np.ascontiguousarray(x)
    T.stub_fn(name)(None, xx.ctypes.data_as(T.u8p), pi.ctypes.data_as(T.f32p), C.byref(v))
    return pi, f32(v.value)


def _expected_priors(mode, a, b):
    """the header's table for the modes that do not draw from the hash stream"""
    i = np.arange(43)
    if mode == 0:
        return np.where(i == a, 1.0, 0.0).astype(f32)
    if mode == 1:
        return np.where((i == a) | (i == b), 0.5, 0.0).astype(f32)
    if mode == 2:
        return np.ldexp(f32(1), -4 * ((7 * i + a) % 43)).astype(f32)
    if mode == 3:
        return np.ldexp((f32(1) + ((5 * i + b) % 8).astype(f32) / f32(8)).astype(f32), -140 - i % 8).astype(f32)
    if mode == 5:
        return np.full(43, f32(1) / f32(43), f32)
    if mode == 6:
        return np.zeros(43, f32)
    if mode == 7:
        return np.ldexp(f32(1), -((11 * i + b) % 43)).astype(f32)
    return None


def test_the_stub_is_what_its_header_says(orc):
    """every mode and every value kind occurs over 512 golden boards and is the table of oracle/azr_oracle.h bit for bit; modes 2 and
    3 hold fp32 denormals, mode 2 exact zeros beside them"""
    x = T.distinct_boards(512)
    modes, vms, denormal = set(), set(), set()
    values = {0: f32(1), 1: f32(-1), 2: f32(0), 3: f32(0.99999994), 4: f32(-0.99999994)}
    for row in x:
        mode, a, b, vm = _draw(row)
        pi, v = _stub("orc_sharp_eval", row)
        modes.add(mode); vms.add(vm)
        want = _expected_priors(mode, a, b)
        if want is not None:
            assert (pi.view(np.uint32) == want.view(np.uint32)).all(), (mode, a, b)
        else:   # orc_hash_eval's formula on the stream after r: strictly positive, near uniform, sums to 1
            assert (pi > 0.5 / 64.5).all() and (pi < 1.5 / 21.5).all() and abs(float(pi.sum()) - 1) < 1e-5
        if vm in values:
            assert v.view(np.uint32) == values[vm].view(np.uint32), (vm, v)
        else:
            assert -1 <= v < 1
        assert (pi >= 0).all() and np.isfinite(pi).all()
        if ((pi > 0) & (pi < T.FLT_MIN)).any():
            denormal.add(mode)
    assert modes == set(range(8)) and vms == set(range(6))
    assert denormal == {2, 3}   # (mode 7 ends at 2^-42: tiny normals, eleven binades under an fp32 ulp of its largest prior)


def test_all_zero_legal_priors_after_normalize(orc):
    """mode 6, and a one-hot whose peak is illegal: orc_normalize finds a zero sum, skips its division and leaves zeros"""
    x = T.distinct_boards(512)
    seen = set()
    for row in x:
        mode, a, b, vm = _draw(row)
        if mode not in (0, 6):
            continue
        pi, _ = _stub("orc_sharp_eval", row)
        valid = M64 & ~(1 << a) & ((1 << 43) - 1) if mode == 0 else (1 << 43) - 1
        orc.orc_normalize(T.ptr(pi), valid)
        assert (pi.view(np.uint32) == 0).all()
        seen.add(mode)
    assert seen == {0, 6}
    pi = np.ldexp(f32(1), -140 - np.arange(43) % 8).astype(f32)   # a denormal sum: the division runs on denormals and gives normals
    orc.orc_normalize(T.ptr(pi), 0b1011)
    assert abs(float(pi.sum()) - 1) < 1e-6 and (pi[[0, 1, 3]] > 0.05).all() and pi[2] == 0


# (simulations, search threads, decisions): the searches of tests/test_gpu_sharp_search.py and a long one
SEARCHES = [(24, 1, 6), (25, 2, 6), (102, 4, 3), (100, 1, 3)]


def _roots(sims, threads, decisions):
    run = T.orc_tree_run(sims, threads, stub="orc_sharp_eval")
    a = run["alive"][:decisions]
    return run["valid"][:decisions][a], run["n"][:decisions][a], run["q"][:decisions][a], run["p"][:decisions][a], run["pi"][:decisions][a]


@pytest.mark.parametrize("sims,threads,decisions", SEARCHES)
def test_the_oracle_search_is_in_the_sharp_regime(orc, sims, threads, decisions):
    """the guard of the GPU tests, on the oracle alone: shares printed, and every search finite with a policy over the legal moves"""
    valid, n, q, p, pi = _roots(sims, threads, decisions)
    T.assert_sharp_regime(T.sharp_census(n, q, p))
    assert np.isfinite(q).all() and np.isfinite(pi).all() and np.isfinite(p).all()
    for i in range(len(valid)):
        ok = T.bits(valid[i])
        assert (pi[i][~ok] == 0).all() and abs(float(pi[i].sum()) - 1) < 1e-6
        assert n[i].sum() >= sims - sims % threads   # (this search's visits, and what tree reuse brought along)
        assert orc.orc_pick_highest(T.ptr(pi[i].copy())) < 43


@pytest.mark.parametrize("threads", [1, 2])
def test_playout_cap_neutral_is_the_oracle_game(orc, threads):
    cfg = T.default_settings(mcts_simulations=6, max_game_rounds=36, mcts_threads=threads)
    ev = orc.orc_sharp_eval
    for seed in range(4242, 4246):
        want, st, sims = PC.oracle_game(cfg, seed, ev)
        got, kinds, gst, gsims = PC.selfplay_game(cfg, seed, ev, 1.0, 2, 99)
        assert got.tobytes() == want.tobytes() and gst == st and gsims == sims and kinds.all()
        on, kinds, _, _ = PC.selfplay_game(cfg, seed, ev, 0.5, 2, 99)   # the cap on: a fast budget of 2 on the same outputs
        pi = on[:, 93:265].copy().view(f32)
        assert len(on) == kinds.sum() > 0 and np.isfinite(pi).all() and (pi >= 0).all() and (np.abs(pi.sum(1) - 1) < 1e-6).all()


@pytest.mark.parametrize("threads", [1, 2])
def test_arena_budget_neutral_is_the_oracle_arena(orc, threads):
    cfg = T.default_settings(mcts_simulations=9, mcts_threads=threads, max_game_rounds=40)
    ev = orc.orc_sharp_eval
    want = T.orc_play_games2(AB.AZ_A, AB.AZ_B, 4, True, 5200, cfg, ev, ev)
    r6, st, rd, fin, games, sims = AB.play_games(AB.AZ_A, AB.AZ_B, 4, True, 5200, cfg, cfg, ev, ev)
    assert tuple(r6) == tuple(want[0]) and (st == want[1]).all() and (rd == want[2]).all() and fin.tobytes() == want[3].tobytes()
    assert [g.tobytes() for g in games] == [g.tobytes() for g in want[4]] and sims > 0
    fast = T.default_settings(mcts_simulations=4, mcts_threads=threads, max_game_rounds=40, hp_exploration=2.0)
    _, _, _, _, games, _ = AB.play_games(AB.AZ_A, AB.AZ_B, 2, True, 5200, cfg, fast, ev, ev)   # another budget on side B
    for g in games:
        pi = g[:, 93:265].copy().view(f32)
        assert len(g) > 0 and np.isfinite(pi).all() and (np.abs(pi.sum(1) - 1) < 1e-6).all()


def test_row_restatements_on_sharp_roots(orc):
    """forced playouts, value mix and surprise weighting on the roots of the (24, 1) search"""
    valid, n, q, p, pi = _roots(24, 1, 6)
    cfg = T.default_settings()
    eps, hp = cfg.dir_noise_epsi, cfg.hp_exploration
    eta = np.full(43, cfg.dir_noise_value, f32)
    z = np.where(np.arange(len(valid)) % 2 == 0, f32(1), f32(-1)).astype(f32)
    saturated = 0
    for i in range(len(valid)):
        ok = T.bits(valid[i])
        order = lambda v=valid[i]: FP.umap_order(orc, v)   # noqa: E731
        # forced playouts: factor 0 is the plain selection and prunes nothing; factor 2 picks a legal move and keeps a policy
        assert FP.forced_pick(n[i], q[i], p[i], valid[i], eta, eps, hp, 0.0, order) == FP.puct_pick(n[i], q[i], p[i], valid[i], eta, eps, hp, order)
        assert not FP.forced_mask(n[i], p[i], valid[i], eta, eps, 0.0).any()
        assert ok[FP.forced_pick(n[i], q[i], p[i], valid[i], eta, eps, hp, 2.0, order)]
        pruned = FP.prune_counts(n[i], q[i], p[i], valid[i], eta, eps, hp, 2.0)
        assert (pruned <= n[i]).all() and pruned.sum() > 0 and pruned[n[i].argmax()] == n[i].max()
        pol = FP.root_policy(pruned, valid[i])
        assert np.isfinite(pol).all() and (pol[~ok] == 0).all() and abs(float(pol.sum()) - 1) < 1e-6
        assert (FP.root_policy(n[i], valid[i]).view(np.uint32) == pi[i].view(np.uint32)).all()
        # value mix: share 0 leaves z, share 1 is the clamped root value
        rq, has = VM.root_value(n[i], q[i], valid[i])
        assert has and -1 <= rq <= 1
        assert VM.blend(z[i], rq, has, 0.0) == z[i] and VM.blend(z[i], rq, has, 1.0) == rq
        saturated += abs(rq) == 1
        # surprise: ln32 clamps a zero or denormal prior at FLT_MIN, so the surprise is finite and not negative
        kl = SU.record_kl(pi[i], p[i], valid[i])
        assert np.isfinite(kl) and kl >= 0
    assert saturated >= 1   # (a root whose every visit came back as the same +-1)
    kl = np.array([SU.record_kl(pi[i], p[i], valid[i]) for i in range(32)], f32)
    assert (SU.game_weights(kl, 0.0, 4.0) == 1).all()
    w = SU.game_weights(kl, 0.75, 4.0)
    assert np.isfinite(w).all() and (w <= 4).all() and (w >= 0.25).all()


# ---- the oracle's own games from the late golden positions, and every option restatement on their decisions ---------------------------
CV, CS = 50.0, 0.5
_late = {}


def _late_game(orc, g, threads, sims=8):
    """the oracle's self-play loop (orc_selfplay_game's body, as tests/test_gpu_mcts.py composes it from a given state) from late
    position g under orc_sharp_eval: per decision the legal moves, N, Q, P, the policy, the net's value of the root, the mover and
    the move; the records with z; the status.  Computed once per (g, threads)."""
    if (g, threads) in _late:
        return _late[g, threads]
    states, rngs = SR.late_positions()
    cfg = T.default_settings(mcts_simulations=sims, mcts_threads=threads)
    ev = C.cast(orc.orc_sharp_eval, C.c_void_p)
    s, r = T.OrcState(), T.OrcRng()
    orc.orc_state_unpack(C.byref(s), T.ptr(states[g]))
    r.x = int(rngs[g])
    m = orc.orc_mcts_create(C.byref(cfg))
    rows, gs = [], orc.orc_game_status(C.byref(s), C.byref(cfg))
    while gs == -1:
        valid = orc.orc_valid_moves(C.byref(s), C.byref(cfg))
        assert orc.orc_mcts_simulate(m, C.byref(s), C.byref(r), ev, None) == 0
        n, q, p, pi = np.zeros(43, np.uint32), np.zeros(43, f32), np.zeros(43, f32), np.zeros(43, f32)
        assert orc.orc_mcts_root_stats(m, C.byref(s), T.ptr(n), T.ptr(q), T.ptr(p), None) == 0
        assert orc.orc_mcts_policy(m, C.byref(s), T.ptr(pi)) == 0
        mv = orc.orc_pick_highest(T.ptr(pi)) if s.round > cfg.temperature_threshold else orc.orc_pick_random(T.ptr(pi), C.byref(r))
        rec = np.zeros(265, np.uint8)
        rec[0] = s.cur
        orc.orc_encode(C.byref(s), T.ptr(rec[1:89]))
        rec[93:265] = pi.view(np.uint8)
        _, vhat = _stub("orc_sharp_eval", rec[1:89])
        rows.append(dict(valid=valid, n=n, q=q, p=p, pi=pi, vhat=vhat, cur=int(s.cur), mv=mv, rec=rec))
        assert orc.orc_make_move(C.byref(s), mv, C.byref(r), C.byref(cfg)) == 0
        gs = orc.orc_game_status(C.byref(s), C.byref(cfg))
        assert len(rows) < 2000
    orc.orc_mcts_destroy(m)
    z = np.array([SR.outcome_z(gs, row["cur"]) for row in rows], f32)
    for row, zr in zip(rows, z):
        row["rec"][89:93] = np.array([zr], f32).view(np.uint8)
    _late[g, threads] = (rows, z, gs)
    return _late[g, threads]


def _is_policy(pi, valid):
    ok = T.bits(valid)
    return bool(np.isfinite(pi).all() and (pi[~ok] == 0).all() and (pi >= 0).all() and abs(float(pi.astype(np.float64).sum()) - 1) <= 43 * 2.0 ** -24)


@pytest.mark.parametrize("threads", [1, 2])
def test_option_restatements_on_the_oracles_late_games(orc, threads):
    """the four late golden games, played by the oracle under orc_sharp_eval.  Neutral (factor 0, share 0, a threshold no value is
    below) every restatement gives the oracle's game back: its policy bit for bit, its z, one copy of every record, no resignation.
    On, every decision gets a policy that sums to 1 over the legal moves and is 0 elsewhere, and a legal move — never NONE."""
    cfg = T.default_settings()
    eps, hp = cfg.dir_noise_epsi, cfg.hp_exploration
    eta = np.full(43, cfg.dir_noise_value, f32)
    zero_rows = saturated = resigned = 0
    for g in range(4):
        rows, z, status = _late_game(orc, g, threads)
        assert len(rows) > 0 and status != -1
        q_series, has_series = [], []
        for d, row in enumerate(rows):
            valid, n, q, p, pi = row["valid"], row["n"], row["q"], row["p"], row["pi"]
            ok = T.bits(valid)
            assert ok.any() and ok[row["mv"]] and _is_policy(pi, valid)
            zero_rows += int((p == 0).all())
            saturated += int(((n > 0) & (np.abs(q) == 1)).any())
            order = lambda v=valid: FP.umap_order(orc, v)   # noqa: E731
            # forced playouts and pruning: factor 0 is the oracle's policy bit for bit; factor 2 keeps a policy and a legal pick
            assert (FP.root_policy(FP.prune_counts(n, q, p, valid, eta, eps, hp, 0.0), valid).view(np.uint32) == pi.view(np.uint32)).all()
            assert FP.forced_pick(n, q, p, valid, eta, eps, hp, 0.0, order) == FP.puct_pick(n, q, p, valid, eta, eps, hp, order)
            assert _is_policy(FP.root_policy(FP.prune_counts(n, q, p, valid, eta, eps, hp, 2.0), valid), valid)
            assert ok[FP.forced_pick(n, q, p, valid, eta, eps, hp, 2.0, order)]
            # value mix: share 0 is the oracle's z
            rq, has = VM.root_value(n, q, valid)
            q_series.append(rq); has_series.append(has)
            assert VM.blend(z[d], rq, has, 0.0).view(np.uint32) == z[d].view(np.uint32) and -1 <= VM.blend(z[d], rq, has, 0.5) <= 1
            # the Gumbel search's record and move, and the tree selection, from these rows
            gum = GU.draw(4242, 9100 + g, d, valid)
            gpi, qhat = GU.policy(n, q, p, row["vhat"], valid, CV, CS)
            assert _is_policy(gpi, valid) and np.isfinite(qhat).all() and np.isfinite(gum).all()
            mv = GU.move(n, np.zeros(43, np.uint32), q, p, gum, row["vhat"], valid, CV, CS)
            assert mv != GU.NONE and ok[mv]
            tmv, score = GT.select_tree(n, np.zeros(43, np.uint32), q, p, row["vhat"], valid, CV, CS)
            assert tmv != GU.NONE and ok[tmv] and np.isfinite(score).all()
        # surprise weighting: share 0 writes every record once; on, the weights are finite and within the cap
        kl = np.array([SU.record_kl(row["pi"], row["p"], row["valid"]) for row in rows], f32)
        assert np.isfinite(kl).all() and (kl >= 0).all()
        assert (SU.game_copies(kl, 0.0, 4.0, 31, 9100 + g)[1] == 1).all()
        w, copies = SU.game_copies(kl, 0.75, 4.0, 31, 9100 + g)
        assert np.isfinite(w).all() and (w <= 4).all() and (copies <= 4).all()
        # resignation: a threshold below every value never cuts the game; q_resign = -0.9 with streak 1 cuts it at a decision it has
        players = [row["cur"] for row in rows]
        assert RS.first_resign(q_series, has_series, players, -2.0, 1) == (-1, RS.NONE)
        cut, who = RS.first_resign(q_series, has_series, players, -0.9, 1)
        assert -1 <= cut < len(rows) and (cut < 0) == (who == RS.NONE)
        resigned += cut >= 0
    print("late games T=%d: zero legal prior rows %d, roots with a visited |Q| == 1 %d, games that resign at -0.9 %d" % (
        threads, zero_rows, saturated, resigned))
    assert zero_rows > 0 and saturated > 0
