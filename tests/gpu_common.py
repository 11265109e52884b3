"""shared helpers for the -m gpu tests (they call the product only through the C-ABI binding)."""
import ctypes as C
import importlib
import os
import sys

import numpy as np

import azr_testlib as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pkg():
    return importlib.import_module("alphazero-risk_amd")


def have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


# ---- the host-stepped PUCT search against the oracle, decision by decision ---------------------------------------------------------------
def search_decisions(orc, stub_name, sims, threads, states, decisions, census=None, **kw):
    """`decisions` host-stepped searches and moves per state (tree reuse, sampling on odd steps) on the engine and in the oracle, both
    served by the oracle's stub net `stub_name`: N, Q, P, the policy, the move, the next state and the RNG bit for bit.  `census`: a
    list that receives the oracle's (N, Q, P) of every searched root."""
    stub = T.stub_fn(stub_name)
    G = len(states)
    cfg = T.default_settings(mcts_simulations=sims, mcts_threads=threads, **kw)
    eng = pkg().Engine(G, blocks=1, sims=sims, dtype=pkg().NET_F32, threads=threads, **kw)
    eng.set_states(states)
    seeds = np.arange(500, 500 + G, dtype=np.uint32)
    eng.set_rng(seeds)
    S, R, M = [], [], []
    for g in range(G):
        s, r = T.OrcState(), T.OrcRng()
        orc.orc_state_unpack(C.byref(s), T.ptr(states[g]))
        r.x = int(seeds[g])
        S.append(s); R.append(r); M.append(orc.orc_mcts_create(C.byref(cfg)))
    evalfn = C.cast(stub, C.c_void_p)
    d = np.zeros(160, np.uint8)
    for step in range(decisions):
        status = eng.status()
        T.host_stub_search(eng, orc, stub)
        n_gpu, q_gpu, p_gpu = eng.root_stats()
        pi_gpu = eng.policy()
        sample = step % 2 == 1
        moves = eng.pick(sample=sample)
        moves[status != -1] = 255
        assert (eng.make_moves(moves) == 0).all()
        after, rng_after = eng.get_states(), eng.get_rng()
        n, q, p, pi = (np.zeros(43, np.uint32), np.zeros(43, np.float32), np.zeros(43, np.float32),
                       np.zeros(43, np.float32))
        for g in range(G):
            if status[g] != -1:
                continue
            assert orc.orc_mcts_simulate(M[g], C.byref(S[g]), C.byref(R[g]), evalfn, None) == 0
            orc.orc_mcts_root_stats(M[g], C.byref(S[g]), T.ptr(n), T.ptr(q), T.ptr(p), None)
            if census is not None:
                census.append((n.copy(), q.copy(), p.copy()))
            assert (n == n_gpu[g]).all(), (step, g, n, n_gpu[g])
            assert (q.view(np.uint32) == q_gpu[g].view(np.uint32)).all(), (step, g)
            assert (p.view(np.uint32) == p_gpu[g].view(np.uint32)).all(), (step, g)
            orc.orc_mcts_policy(M[g], C.byref(S[g]), T.ptr(pi))
            assert (pi.view(np.uint32) == pi_gpu[g].view(np.uint32)).all(), (step, g)
            mv = orc.orc_pick_random(T.ptr(pi), C.byref(R[g])) if sample else orc.orc_pick_highest(T.ptr(pi))
            assert mv == moves[g], (step, g)
            assert orc.orc_make_move(C.byref(S[g]), mv, C.byref(R[g]), C.byref(cfg)) == 0
            orc.orc_state_pack(C.byref(S[g]), T.ptr(d))
            assert (d == after[g]).all(), (step, g)
            assert R[g].x == rng_after[g], (step, g)
    for m in M:
        orc.orc_mcts_destroy(m)
    eng.close()


# ---- whole device-resident self-play games against the oracle ----------------------------------------------------------------------------
def selfplay_games(orc, threads, G=6, flat=None, **kw):
    """G whole games of device-resident self-play (6 simulations, one block, NET_F32; `flat`: the weights, by default those of
    make_net_flat(1, seed=11, perturb_bn=True)) against orc_selfplay_game with the device net called back for every evaluation; returns the counters"""
    sims, B = 6, 1
    P = pkg()
    eng = P.Engine(G, blocks=B, sims=sims, dtype=P.NET_F32, threads=threads, **kw)
    eng.set_weights(T.make_net_flat(B, seed=11, perturb_bn=True) if flat is None else flat)
    base = 4242
    eng.selfplay_start(base)
    for _ in range(400):
        eng.selfplay_run(64)
        c = eng.counters()
        if c["games_finished"] >= G:
            break
    c = eng.counters()
    assert c["games_finished"] >= G and c["errors"] == 0 and c["nodes_dropped"] == 0
    recs = eng.drain()
    assert len(recs) == c["samples"]

    @T.EVAL_FN
    def hip_eval(ctx, in88, pi, v):
        x = np.ctypeslib.as_array(in88, shape=(88,)).copy()[None]
        p, vv = eng.predict(x)
        C.memmove(pi, p.ctypes.data, 43 * 4)
        v[0] = float(vv[0])

    cfg = T.default_settings(mcts_simulations=sims, mcts_threads=threads, **kw)
    # records of one game are contiguous in the ring; games finish in any order: match by content
    want = {}
    for g in range(G):
        buf = np.zeros((4096, 265), np.uint8)
        st, rounds = C.c_int(0), C.c_int(0)
        n = orc.orc_selfplay_game(C.byref(cfg), base + g, hip_eval, None, T.ptr(buf), 4096, C.byref(st),
                                  C.byref(rounds), None, 0, None, None)
        assert n > 0
        want[g] = buf[:n].copy()
    blob = recs.tobytes()
    for g in range(G):
        assert want[g].tobytes() in blob, f"game {g} record stream not found in the device's output"
    eng.close()
    return c


# ---- arena helpers shared by the arena, scripted-samples and dropped-game tests -----------------------------------------------------
def run_arena(eng, k0, k1, total, cap, mirror, base):
    eng.arena_start(k0, k1, total, per_slot_cap=cap, mirror=mirror, base_seed=base)
    for _ in range(2000):
        if eng.arena_run(64):
            break
    else:
        raise AssertionError("arena did not finish")
    return eng.arena_results(), eng.arena_log()


def half_slot(g, G, base):
    """slot g of a G-slot concurrent arena = (half, first pair seed, pair stride) of tests/azr_testlib.orc_play_half_games"""
    return g & 1, base + (g >> 1), G // 2


def arena_play(eng, k0, k1, total, cap, mirror, base, script=False, az=False, chunk=None, sink=None):
    """the whole arena, draining after every run (in pieces of `chunk` records, each handed to `sink` instead of kept when
    given); returns (results, log, records, runs that came back unfinished)"""
    eng.arena_collect_scripted_samples(script)
    eng.arena_collect_samples(az)
    eng.arena_start(k0, k1, total, per_slot_cap=cap, mirror=mirror, base_seed=base)
    out, waits = [], 0
    for _ in range(2000):
        fin = eng.arena_run(64)
        if script or az:
            while True:
                r = eng.drain(chunk) if chunk else eng.drain()
                if len(r):
                    if sink:
                        sink(r)
                    else:
                        out.append(r)
                if not chunk or len(r) < chunk:
                    break
        if fin:
            break
        waits += 1
    else:
        raise AssertionError("arena did not finish")
    rec = np.concatenate(out) if out else np.zeros((0, 265), np.uint8)
    return eng.arena_results(), eng.arena_log(), rec, waits


def concurrent_two_net_arena(orc, threads, b_first, flat_a, flat_b, G=6, S=12, rounds=40, dtype_name="NET_BF16"):
    """two games per slot on G slots in concurrent mirrored pairs between two one-block nets: results, final states, rounds and every
    (s, pi, z) record of both AlphaZero players against the oracle's slots, the two DEVICE nets called back per evaluation; returns the
    counters"""
    fm = T.data_field_mask()
    P = pkg()
    per_slot, B, base = 2, 1, 6100
    a = P.Engine(G, blocks=B, sims=S, dtype=getattr(P, dtype_name), threads=threads, max_game_rounds=rounds)
    b = P.Engine(G, blocks=B, sims=S, dtype=getattr(P, dtype_name), threads=threads, max_game_rounds=rounds)
    a.set_weights(flat_a)
    b.set_weights(flat_b)
    a.arena_set_opponent(b)
    a.arena_collect_samples(True)
    k = (P.PLAYER_ALPHAZERO_B, P.PLAYER_ALPHAZERO) if b_first else (P.PLAYER_ALPHAZERO, P.PLAYER_ALPHAZERO_B)
    res, (n, st, rd, fin) = run_arena(a, k[0], k[1], 10 ** 6, per_slot, P.MIRROR_CONCURRENT, base)
    c = a.counters()
    assert (n == per_slot).all() and c["errors"] == 0 and c["nodes_dropped"] == 0
    recs = a.drain()

    def make_eval(eng):
        @T.EVAL_FN
        def f(ctx, in88, pi, v):
            x = np.ctypeslib.as_array(in88, shape=(88,)).copy()[None]
            p, vv = eng.predict(x)
            C.memmove(pi, p.ctypes.data, 43 * 4)
            v[0] = float(vv[0])
        return f

    ea, eb = make_eval(a), make_eval(b)
    cfg = T.default_settings(mcts_simulations=S, mcts_threads=threads, max_game_rounds=rounds)
    tot = np.zeros(6, np.int64)
    blob = recs.tobytes()
    nrec = 0
    for g in range(G):
        half, q0, stride = half_slot(g, G, base)
        r6, ost, ord_, ofin, orec = T.orc_play_half_games(k[0], k[1], per_slot, half, q0, stride, cfg, ea, eb)
        assert (st[g, :per_slot] == ost).all(), (g, st[g], ost)
        assert (rd[g, :per_slot] == ord_).all(), g
        assert (fin[g, :per_slot][:, fm] == ofin[:, fm]).all(), g
        tot += np.array(r6)
        for gi, game in enumerate(orec):
            assert len(game) > 0 and game.tobytes() in blob, (g, gi)
            nrec += len(game)
    assert nrec == len(recs)
    assert [res["count"], res["draw"], res["win"][0], res["win_and_started"][0], res["win"][1], res["win_and_started"][1]] == list(tot)
    a.arena_set_opponent(None)
    a.close(); b.close()
    return c


# ---- the host-stepped search of the root-noise and forced-playouts tests --------------------------------------------------------------
def host_net(sharp=False):
    """the weights of the host-stepped option tests: make_net_flat(1, seed=23, perturb_bn=True), or the sharp net of that seed with its
    logits scaled by 2^10: at 2^8 the 14 legal moves of these tests' set-up roots all keep a positive prior, at 2^10 every one of the
    eight roots has a legal move with a prior of exactly 0 and four hold a denormal one (the oracle's fp32 net)"""
    return T.make_sharp_net_flat(1, seed=23, kp=10) if sharp else T.make_net_flat(1, seed=23, perturb_bn=True)


def setup_engine(sims, sharp=False):
    P = pkg()
    eng = P.Engine(8, blocks=1, sims=sims, dtype=P.NET_F32, threads=1)
    eng.set_weights(host_net(sharp))
    eng.new_games(np.arange(4100, 4108, dtype=np.uint32))   # setup phase: no descent of 24 ends in a finished game
    return eng


def stepped(eng, eta, passes, check):
    """begin / leaves / azr_nn_predict / apply one pass at a time; check(prev stats, new stats) between consecutive passes"""
    eng.set_root_noise(eta)
    eng.mcts_begin()
    x, need, act = eng.mcts_leaves()          # setRootState's root expansion
    eng.mcts_apply(*eng.predict(x))
    x, need, act = eng.mcts_leaves()          # the root is in the tree, descent 1 waits for the net
    prev = eng.root_stats()
    assert (prev[0] == 0).all()
    for i in range(passes):
        assert act == eng.G
        eng.mcts_apply(*eng.predict(x))
        x, need, act = eng.mcts_leaves()
        cur = eng.root_stats()
        check(i, prev, cur)
        prev = cur
    return prev


def pi_of(rec):
    return rec[:, 93:265].copy().view(np.float32)


def assert_one_hot(rec):
    pi = pi_of(rec)
    assert ((pi == 1.0).sum(1) == 1).all() and ((pi != 0.0).sum(1) == 1).all()


# ---- training records shared by the optimiser-step and validation tests -----------------------------------------------------------------
def records(n, seed=0):
    """synthetic (s, pi, z) records on real encoded positions: pi random over a random support, z in {-1, 0, 1}"""
    g = np.load(os.path.join(T.GOLDEN, "encode.npz"))
    x = g["in88"]
    rng = np.random.default_rng(seed)
    x = x[rng.integers(0, len(x), n)]
    pi = rng.uniform(0.0, 1.0, (n, 43)).astype(np.float32) * (rng.uniform(0, 1, (n, 43)) < 0.3)
    pi[:, 42] += 1e-3
    pi = (pi / pi.sum(1, keepdims=True)).astype(np.float32)
    z = rng.integers(-1, 2, n).astype(np.float32)
    rec = np.zeros((n, 265), np.uint8)
    rec[:, 0] = x[:, 42]
    rec[:, 1:89] = x
    rec[:, 89:93] = z.view(np.uint8).reshape(n, 4)
    rec[:, 93:265] = pi.view(np.uint8).reshape(n, 172)
    return rec
