"""GPU: the Gumbel search's selection below the root (azr_selfplay_set_gumbel_tree, azr_mcts_set_gumbel_tree,
azr_debug_gumbel_tree_select) and the node inspection it is tested through (azr_mcts_node_stats).  The contract is include/azr.h's;
tests/gumbel_tree_ref.py restates the rule in np.float32.  Checked here: the debug kernel against the restatement, bit for bit;
node_stats against root_stats, on unknown states and as a read-only call; every selection of a host-stepped search replayed on the
host at every depth, down to the leaf the device handed out; device self-play against its host-stepped retrace (all five new tree
steps); off is the engine that never called it, and toggling keeps the trees; slot independence; refusals.
Engines of 8 games, one block, NET_F32, budgets of 16 and 32."""
import ctypes as C
import zlib

import numpy as np
import pytest

import azr_testlib as T
import gumbel_ref as G
import gumbel_retrace as GR
import gumbel_tree_ref as GT
import selfplay_retrace as SR
import surprise_ref as S
import value_mix_ref as V
from gpu_common import pi_of, pkg

pytestmark = pytest.mark.gpu
f32 = np.float32
SLOTS = 8
CV, CS, GSEED = GR.CV, GR.CS, GR.GSEED
BASE, QUOTA = 9300, 4
SHARE, MAXW, PSEED, QSHARE = 0.75, 4.0, 31, 0.5
SEEDS = np.arange(4100, 4100 + SLOTS, dtype=np.uint32)


def _engine(threads=1, sims=16):
    P = pkg()
    eng = P.Engine(SLOTS, blocks=1, sims=sims, dtype=P.NET_F32, threads=threads)
    eng.set_weights(T.make_net_flat(1, seed=23, perturb_bn=True))
    return eng


# ---- 1. the debug kernel, bit for bit ------------------------------------------------------------------------------------------------
def test_the_selection_on_the_device_is_the_restatement():
    rows = GT.rows(21, 240) + GT.rows(22, 60, top=300) + [row for _, row, _ in GT.hand_rows()]
    N, act, Q, P, vhat, valid = (np.array([r[k] for r in rows]) for k in range(6))
    want = [GT.select_tree(*r, CV, CS) for r in rows]
    assert [w[0] for w in want][-len(GT.hand_rows()):] == [mv for _, _, mv in GT.hand_rows()]
    eng = _engine()
    mv, score = eng.debug_gumbel_tree_select(CV, CS, N, act, Q, P, vhat.astype(f32), valid.astype(np.uint64))
    eng.close()
    assert mv.tolist() == [w[0] for w in want]
    assert score.tobytes() == np.array([w[1] for w in want]).tobytes(), np.nonzero(score != np.array([w[1] for w in want]))
    assert len(set(mv.tolist())) > 20


# ---- 2. node_stats ---------------------------------------------------------------------------------------------------------------------
def _draws(eng, d):
    return np.array([G.draw(GSEED, int(s), d, int(v)) for s, v in zip(SEEDS, eng.valid_moves())])


def _peaked(x):
    """an evaluator of the host's own, a function of the position alone: a peaked policy (Dirichlet(0.05)) and a value anywhere in
    (-0.9, 0.9).  Under a random net's nearly flat priors and nearly equal values every selection below the root takes a move nobody has
    tried, whatever the rule, and no descent of a budget of 16 or 32 gets past depth 1; these send visits back into the same child."""
    pi, v = np.zeros((len(x), 43), f32), np.zeros(len(x), f32)
    for r, row in enumerate(x):
        rng = np.random.default_rng(zlib.crc32(row.tobytes()))
        pi[r], v[r] = rng.dirichlet(np.full(43, 0.05)), rng.uniform(-0.9, 0.9)
    return pi, v


def _search(eng, g, after_leaves=None, evaluate=None):
    """one host-stepped search under the vectors g, the leaves evaluated by `evaluate` (none: the engine's net); after_leaves(x, need) is
    called behind every azr_mcts_leaves, before the answers go back.  The leaves every pass handed out: [(need, the needed rows of x)]"""
    eng.set_root_gumbel(g)
    eng.mcts_begin()
    out = []
    while True:
        x, need, act = eng.mcts_leaves()
        out.append((need.tobytes(), x[need].tobytes()))
        if after_leaves:
            after_leaves(x, need)
        if not act:
            return out
        eng.mcts_apply(*(evaluate or eng.predict)(x))


def test_node_stats_on_the_games_own_states_is_root_stats():
    eng = _engine(2, 16)
    eng.new_games(SEEDS)
    eng.set_gumbel(4, CV, CS)
    eng.set_gumbel_tree(1)
    seen = []

    def same(x, need):
        n, act, q, p, vhat, found = eng.node_stats(eng.get_states())
        rn, rq, rp = eng.root_stats()
        assert n.tobytes() == rn.tobytes() and q.tobytes() == rq.tobytes() and p.tobytes() == rp.tobytes()
        assert (found == rp.any(1)).all() and not n[~found].any() and not act[~found].any() and not vhat[~found].any()
        assert (act.sum(1)[found] == need.reshape(SLOTS, 2).sum(1)[found]).all()   # the visits in flight at a root: this pass's descents
        seen.append((int(found.sum()), int(n.sum())))

    for d in range(2):
        _search(eng, _draws(eng, d), same)
        n, act, q, p, vhat, found = eng.node_stats(eng.get_states())
        assert found.all() and (n.sum(1) >= 16).all() and not act.any()
        assert vhat.tobytes() == eng.predict(eng.encode())[1].tobytes()             # the net's value of the root, kept where it was expanded
        assert (eng.make_moves(eng.gumbel_pick()) == 0).all()
    assert seen[0] == (0, 0) and max(s[1] for s in seen) >= 16 * SLOTS                  # mid-search: from the empty tree to the full budget
    # a state that was never searched: another game's root
    n, act, q, p, vhat, found = eng.node_stats(np.roll(eng.get_states(), 1, 0))
    assert not found.any() and not n.any() and not act.any() and not q.any() and not p.any() and not vhat.any()
    # the optional outputs may be left out
    st, n2, q2, p2, f2 = eng.get_states(), np.zeros((SLOTS, 43), np.uint32), np.zeros((SLOTS, 43), f32), np.zeros((SLOTS, 43), f32), np.zeros(SLOTS, np.uint8)
    assert eng.L.azr_mcts_node_stats(eng.h, T.ptr(st), T.ptr(n2), None, T.ptr(q2), T.ptr(p2), None, T.ptr(f2)) == 0
    assert n2.tobytes() == eng.root_stats()[0].tobytes() and f2.all()
    eng.close()


def test_node_stats_between_leaves_and_apply_changes_nothing():
    def run(look):
        eng = _engine(2, 16)
        eng.new_games(SEEDS)
        eng.set_gumbel(4, CV, CS)
        eng.set_gumbel_tree(1)
        out = []
        for d in range(2):
            states = eng.get_states()
            other = np.roll(states, 1, 0)
            out += _search(eng, _draws(eng, d), (lambda x, need: (eng.node_stats(states), eng.node_stats(other))) if look else None)
            out += [a.tobytes() for a in eng.root_stats()] + [eng.get_rng().tobytes(), eng.get_states().tobytes(), eng.gumbel_policy()[0].tobytes()]
            assert (eng.make_moves(eng.gumbel_pick()) == 0).all()
        eng.close()
        return out

    assert run(True) == run(False)


# ---- 3. every selection of a host-stepped search, at every depth ---------------------------------------------------------------------
class _Replay:
    """the descents of every pass of one search, replayed on the host.  `rul` serves as the rules: set_states -> make_moves -> get_states
    / encode / valid_moves.  In the set-up phase moves are deterministic and no descent ends a game, so every descent ends in a leaf."""

    def __init__(self, eng, rul, g, m, n):
        self.eng, self.rul, self.g, self.m, self.n = eng, rul, g, m, n
        self.root = eng.get_states()
        self.N0 = None
        self.claims = np.zeros(SLOTS, np.int64)
        self.deep1 = self.deep2 = 0
        self.top = 0.0

    def __call__(self, x, need):
        """behind a pass: the rows on the device are the rows its descents saw (completed N and Q move only where a pass consumes the
        net's answers, in front of its descents); the visits in flight are this pass's own and are counted here, thread by thread"""
        Tn, need = self.eng.T, need.reshape(SLOTS, self.eng.T)
        rootN, in_tree = self.eng.node_stats(self.root)[::5]
        if self.N0 is None:                                                         # the first pass consumes nothing: the rows the search began on
            self.N0 = rootN.copy()                                                   # (zeros for a root that is not in the tree)
        searching = in_tree & (self.claims < self.n)
        # the precondition: a root that is not in the tree asks for itself, a searching game hands out T leaves, a finished one none
        assert (need[~in_tree] == ([True] + [False] * (Tn - 1))).all() and need[searching].all() and not need[in_tree & ~searching].any()
        self.rul.set_states(self.root)
        root_code = self.rul.encode()
        for gi in np.nonzero(~in_tree)[0]:
            assert x[gi * Tn].tobytes() == root_code[gi].tobytes()
        inflight = [dict() for _ in range(SLOTS)]                                    # per game: state -> this pass's visits in flight
        for th in range(Tn):
            states, going, leaf = self.root.copy(), searching.copy(), self.root.copy()
            depth = 0
            while going.any():
                self.rul.set_states(states)
                valid = self.rul.valid_moves()
                N, _, Q, P, vhat, found = self.eng.node_stats(states)
                mv = np.full(SLOTS, 255, np.uint8)
                for gi in np.nonzero(going)[0]:
                    if not found[gi]:                                                # the first state that is not in the tree: the leaf
                        going[gi], leaf[gi] = False, states[gi]
                        continue
                    act = inflight[gi].setdefault(states[gi].tobytes(), np.zeros(43, np.uint32))
                    if depth == 0:
                        mv[gi], _ = G.select(N[gi], self.N0[gi], act, Q[gi], P[gi], self.g[gi], vhat[gi], int(valid[gi]),
                                             int(self.claims[gi]) + th, self.m, self.n, CV, CS)
                    else:
                        mv[gi], _ = GT.select_tree(N[gi], act, Q[gi], P[gi], vhat[gi], int(valid[gi]), CV, CS)
                        self.deep1 += 1
                        self.top = max(self.top, float(P[gi].max()))
                        self.deep2 += depth >= 2
                    act[mv[gi]] += 1
                assert (self.rul.make_moves(mv) == 0).all()
                states = self.rul.get_states()
                depth += 1
                assert depth < 64
            self.rul.set_states(leaf)
            code = self.rul.encode()
            for gi in np.nonzero(searching)[0]:
                assert x[gi * Tn + th].tobytes() == code[gi].tobytes(), (gi, th, int(self.claims[gi]))
        self.claims[searching] += Tn


@pytest.mark.parametrize("threads,m,n", [(1, 4, 16), (2, 4, 16), (2, 16, 32)])
def test_every_selection_of_a_host_stepped_search_is_the_restatement(threads, m, n):
    every_selection_is_the_restatement(threads, m, n, _peaked)


def _sharp(x):
    """the oracle's sharp stub as the host's evaluator: priors of exactly 0 and 1, denormal priors, values of +-1"""
    stub = T.stub_fn("orc_sharp_eval")
    pi, v, vv = np.zeros((len(x), 43), f32), np.zeros(len(x), f32), C.c_float(0)
    for r in range(len(x)):
        stub(None, x[r].ctypes.data_as(T.u8p), pi[r].ctypes.data_as(T.f32p), C.byref(vv))
        v[r] = vv.value
    return pi, v


def test_sharp_every_selection_of_a_host_stepped_search_is_the_restatement():
    """the smallest shape with the leaves evaluated by orc_sharp_eval: the improved policy of rows whose priors are all zero (every
    logit at the FLT_MIN clamp) and whose completed Q are +-1"""
    every_selection_is_the_restatement(1, 4, 16, _sharp)


def every_selection_is_the_restatement(threads, m, n, evaluate):
    eng, rul, plain = _engine(threads, n), _engine(threads, n), _engine(threads, n)
    for e in (eng, plain):
        e.new_games(SEEDS)                                                          # set-up phase
        e.set_gumbel(m, CV, CS)
    eng.set_gumbel_tree(1)
    deep1 = deep2 = 0
    for d in range(3):
        g, rng = _draws(eng, d), eng.get_rng()
        replay = _Replay(eng, rul, g, m, n)
        leaves = _search(eng, g, replay, evaluate)
        assert (replay.claims == n).all() and eng.get_rng().tobytes() == rng.tobytes()   # no dice were thrown: nothing random in a descent
        deep1, deep2 = deep1 + replay.deep1, deep2 + replay.deep2
        if d == 0:   # the same games from the same empty trees under PUCT below the root
            differ = _search(plain, g, None, evaluate) != leaves
        assert (eng.make_moves(eng.gumbel_pick()) == 0).all()
    print("largest prior met below the root in the last decision: %.3f" % replay.top)
    print("selections checked at depth >= 1: %d, at depth >= 2: %d; the first decision's leaves differ from PUCT's: %s" % (deep1, deep2, differ))
    assert deep1 > 0 and (evaluate is _sharp or (deep2 > 0 and differ))   # (on the sharp stub depth 2 and the difference are printed only)
    for e in (eng, rul, plain):
        e.close()


# ---- 4. device self-play is the host-stepped retrace -----------------------------------------------------------------------------------
@pytest.mark.parametrize("m,threads,sims,psw,mix", [(4, 1, 16, False, False), (4, 2, 16, False, False), (16, 2, 32, False, False),
                                                    (4, 2, 16, True, False), (4, 2, 16, False, True), (4, 2, 16, True, True)])
def test_selfplay_is_the_host_stepped_retrace(m, threads, sims, psw, mix):
    run = SR.Run(BASE, QUOTA, threads, sims, surprise=(SHARE, MAXW, PSEED) if psw else None, value_mix=QSHARE if mix else None)
    recs, c, rng_dev = GR.selfplay(run, m, 1)
    games, tot, rng_ref = GR.retrace(run, m, 1)
    print("records per game:", [len(g.records) for g in games], tot)
    streams = []
    for g, game in enumerate(games):
        want, copies = game.records, None
        if psw:
            kl = np.array([S.record_kl(pi, pr, va) for pi, pr, va in zip(pi_of(game.records), game.prior, game.valid)], f32)
            copies = S.game_copies(kl, SHARE, MAXW, PSEED, BASE + g)[1]
        if mix:
            want = want.copy()
            for r in range(len(want)):
                q, has = V.root_value(game.N[r], game.Q[r], game.valid[r])
                want[r, 89:93] = np.array([V.blend(game.z[r], q, has, QSHARE)], f32).view(np.uint8)
        streams.append((want, copies))
    if psw:
        tot = dict(tot, samples=sum(int(np.sum(cp)) for _, cp in streams))
    SR.assert_streams(recs, c, streams, tot)
    assert rng_dev == rng_ref, (rng_dev, rng_ref)                                   # the dice streams after the last move
    pi = pi_of(recs)
    assert np.abs(pi.astype(np.float64).sum(1) - 1).max() <= 43 * 2.0 ** -24
    if not psw and not mix:   # the flag is in force: PUCT below the root writes other records
        assert GR.selfplay(run, m, 0)[0].tobytes() != recs.tobytes()


# ---- 5. off is the engine that never called it -----------------------------------------------------------------------------------------
def test_off_is_the_engine_that_never_called_it():
    def two_decisions(touch, toggle=False):
        eng = _engine(2, 16)
        eng.new_games(SEEDS)
        eng.set_gumbel(4, CV, CS)
        touch(eng)
        out, reused = [], 0
        for d in range(2):
            eng.set_root_gumbel(_draws(eng, d))
            if toggle:
                eng.set_gumbel_tree(1 - d)
                eng.mcts_begin()
                reused += int(eng.root_stats()[0].any(1).sum())                     # N0 != 0: a root that tree reuse brought along
            _search(eng, eng.root_gumbel(), None, _peaked)
            mv = eng.gumbel_pick()
            out += [a.tobytes() for a in eng.root_stats()] + [eng.gumbel_policy()[0].tobytes(), mv.tobytes(), eng.get_rng().tobytes()]
            assert (eng.make_moves(mv) == 0).all()
        eng.close()
        return out, reused

    never = two_decisions(lambda eng: None)[0]
    assert never == two_decisions(lambda eng: eng.set_gumbel_tree(0))[0]
    assert never == two_decisions(lambda eng: (eng.set_gumbel_tree(1), eng.set_gumbel_tree(0)))[0]
    on = two_decisions(lambda eng: eng.set_gumbel_tree(1))[0]
    assert never != on
    # toggling between two decisions keeps the trees: the second decision's roots come with their visits
    toggled, reused = two_decisions(lambda eng: None, toggle=True)
    assert reused > 0 and toggled[:6] == on[:6]
    # azr_mcts_set_gumbel(h, 0, ...) puts it back to 0: the next Gumbel search is the plain one
    assert never == two_decisions(lambda eng: (eng.set_gumbel_tree(1), eng.set_gumbel(0, CV, CS), eng.set_gumbel(4, CV, CS)))[0]


@pytest.mark.parametrize("m", [0, 4])
def test_a_quota_with_the_flag_off_is_the_one_that_never_called_it(m):
    """without the Gumbel search, and under it with the flag 0"""
    never = SR.quota_on_slots((8,), lambda eng: eng.selfplay_set_gumbel(m, CV, CS, GSEED), 16, BASE, games=4)
    called = _quota(8, 0) if m else SR.quota_on_slots((8,), lambda eng: eng.selfplay_set_gumbel_tree(0), 16, BASE, games=4)
    assert never[0].tobytes() == called[0].tobytes() and never[1:] == called[1:]
    if m:
        assert _quota(8, 1)[0].tobytes() != never[0].tobytes()


# ---- 6. slot independence --------------------------------------------------------------------------------------------------------------
_quotas = {}


def _quota(slots, tree):
    """SR.quota_on_slots' quota under the Gumbel search on `slots` slots (one run per slot count, flag and process)"""
    if (slots, tree) not in _quotas:
        _quotas[slots, tree] = SR.quota_on_slots((slots,), GR.configure(4, tree), 16, BASE, games=4)
    return _quotas[slots, tree]


@pytest.mark.parametrize("slots", [2, 4])
def test_a_quota_writes_the_same_records_as_on_eight_slots(slots):
    recs, dec, sims, samples = _quota(8, 1)
    other = _quota(slots, 1)
    assert samples == dec and other[0].tobytes() == recs.tobytes() and other[1:] == (dec, sims, samples)


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------
def test_argument_and_combination_refusals():
    P = pkg()
    eng = _engine(2, 16)
    L = eng.L
    assert L.azr_selfplay_set_gumbel_tree(None, 1) == 3 and L.azr_mcts_set_gumbel_tree(None, 1) == 3                 # AZR_E_BAD_HANDLE
    assert L.azr_mcts_node_stats(None, None, None, None, None, None, None, None) == 3
    assert L.azr_debug_gumbel_tree_select(None, CV, CS, None, None, None, None, None, None, 0, None, None) == 3
    assert L.azr_mcts_node_stats(eng.h, None, None, None, None, None, None, None) == 1                                # AZR_E_INVALID_ARGUMENT
    eng.set_gumbel(4, CV, CS)
    for setter, name in ((eng.selfplay_set_gumbel_tree, "azr_selfplay_set_gumbel_tree"), (eng.set_gumbel_tree, "azr_mcts_set_gumbel_tree")):
        for bad in (2, -1, 255):
            with pytest.raises(P.AzrError) as e:
                setter(bad)
            assert e.value.code == 1 and name in str(e.value), bad
        setter(1); setter(0)
    # the host-stepped setter without a host-stepped Gumbel search
    eng.set_gumbel(0, CV, CS)
    for on in (0, 1):
        with pytest.raises(P.AzrError) as e:
            eng.set_gumbel_tree(on)
        assert e.value.code == 1 and "azr_mcts_set_gumbel" in str(e.value)
    # self-play with the flag and m = 0: refused at the start, both setters named, and the handle goes on as it was
    eng.new_games(SEEDS)
    eng.simulate()
    before = [a.tobytes() for a in eng.root_stats()] + [eng.get_states().tobytes(), eng.get_rng().tobytes()]
    eng.selfplay_set_gumbel_tree(1)
    for start in (lambda: eng.selfplay_start(BASE), lambda: eng.selfplay_start_games(BASE, 2)):
        with pytest.raises(P.AzrError) as e:
            start()
        assert e.value.code == 1 and "azr_selfplay_set_gumbel_tree" in str(e.value) and "azr_selfplay_set_gumbel " in str(e.value)
    assert before == [a.tobytes() for a in eng.root_stats()] + [eng.get_states().tobytes(), eng.get_rng().tobytes()]
    eng.selfplay_set_gumbel(4, CV, CS, GSEED)
    eng.selfplay_start_games(BASE, 2)
    eng.selfplay_run(4)
    assert eng.root_gumbel().any() and eng.counters()["errors"] == 0
    with pytest.raises(P.AzrError):                                                 # a running self-play ended the host-stepped options
        eng.set_gumbel_tree(1)
    eng.close()
