"""GPU: the value mix of the self-play records (azr_selfplay_set_value_mix, azr_mcts_root_value, azr_debug_value_mix).  The contract is
include/azr.h's; tests/value_mix_ref.py restates it in np.float32.  Checked here: the rule on the device against the restatement, bit
for bit; azr_mcts_root_value against the restatement on azr_mcts_root_stats' rows; device self-play against the same games retraced
decision by decision through the host-stepped entry points with z' filled in by the restatement (plain at one and two search threads,
with a playout cap, Dirichlet noise, forced playouts and pruning, and that again under surprise weighting: both flush paths); the mix
on against off; slot independence; off is the engine that never called it; the arena never sees it; argument checks.
Engines of 8 games, one block, NET_F32, 8 simulations, on the late golden positions of tests/selfplay_retrace.py."""
import numpy as np
import pytest

import selfplay_retrace as SR
import surprise_ref as S
import value_mix_ref as V
from gpu_common import arena_play, pi_of, pkg

pytestmark = pytest.mark.gpu
f32 = np.float32
G = 8
BASE, NSEED, CSEED, SIMS, FAST, ALPHA, K, QUOTA = 9100, 77, 99, 8, 4, 0.3, 2.0, 4
SHARE, MAXW, PSEED = 0.75, 4.0, 31                  # surprise weighting, as in test_gpu_surprise_weighting
QSHARE = 0.5
ALL = (1 << 43) - 1
OVER_ONE_SEED = 6                                   # _over_one_row: the first seed whose num / den exceeds 1 (searched on the CPU)


# ---- 1. the rule, bit for bit ------------------------------------------------------------------------------------------------------
def _over_one_row(seed):
    """43 legal moves, N up to 2^24 - 1, Q of 1, one ulp below and one ulp above.  With |Q| <= 1 the clamp cannot act: a term N * Q is
    then at most N, rounding is monotone, so every partial sum of num stays at or below den's.  An incrementally updated mean can end
    one ulp past 1, and with such a Q num / den can: the clamp is for that."""
    rng = np.random.default_rng(seed)
    N = rng.integers(1, 1 << 24, 43).astype(np.uint32)
    Q = rng.choice(np.array([1.0, 1 - 2.0 ** -24, 1 + 2.0 ** -23], f32), 43, p=[0.6, 0.3, 0.1])
    return N, Q


def _rule_rows():
    """(N [130, 43], Q, valid [130], z [130]): the special rows first, random ones behind them; z cycles through -1, 0, 1"""
    rng = np.random.default_rng(23)
    rows = []

    def add(N, Q, valid):
        rows.append((np.asarray(N, np.uint32), np.asarray(Q, f32), int(valid)))

    def rnd(nmax=40):
        return rng.integers(1, nmax, 43).astype(np.uint32), rng.uniform(-1, 1, 43).astype(f32)

    N, Q = rnd(); add(N, Q, 1 << 17)                                  # one legal move
    N, Q = rnd(); add(N, Q, ALL)                                      # all 43 legal
    N, Q = rnd(); add(np.zeros(43), Q, ALL)                           # N zero everywhere: has_q 0, z' = z
    N, Q = rnd(); N[::2] = 0; add(N, Q, ALL)                          # N zero on some legal moves
    N, Q = rnd(); N[:40] = 0; add(N, Q, ALL & ~(7 << 40))             # N zero on EVERY legal move, visits under illegal ones only
    for sign in (1, -1):                                              # Q = +-1 exactly, against z (set below)
        N, Q = rnd(); add(N, np.full(43, sign), ALL)
    N, Q = rnd(); N[[3, 8, 21, 30, 42]] = (1 << 24) - np.array([1, 2, 3, 5, 1]); add(N, Q, ALL)   # den rounds
    N, Q = rnd(1 << 24); add(N, Q, ALL)
    N, Q = _over_one_row(OVER_ONE_SEED); add(N, Q, ALL)               # num / den above 1 before the clamp
    add(N, -Q, ALL)                                                   # ... and below -1
    for junk in (np.nan, np.inf, -3e38):                              # junk N and Q under illegal moves
        N, Q = rnd()
        valid = sum(1 << m for m in range(43) if rng.random() < 0.4) | 1
        bad = ~V.bits(valid)
        N[bad] = rng.integers(0, 1 << 32, bad.sum(), dtype=np.uint64).astype(np.uint32)
        Q[bad] = junk
        add(N, Q, valid)
    special = len(rows)
    while len(rows) < 130:
        N, Q = rnd(300)
        N[rng.random(43) < 0.5] = 0
        add(N, Q, sum(1 << m for m in range(43) if rng.random() < 0.5) or 1)
    z = np.array([(-1.0, 0.0, 1.0)[i % 3] for i in range(130)], f32)
    z[5], z[6] = -1.0, 1.0                                            # Q = +1 with z = -1, Q = -1 with z = +1
    return (np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows], np.uint64), z, special)


@pytest.mark.parametrize("q_share", [0.25, 1.0, 1.0 - 2.0 ** -24])
def test_the_rule_on_the_device_is_the_restatement(q_share):
    N, Q, valid, z, special = _rule_rows()
    want_q, want_has, want_z = V.mix_rows(q_share, N, Q, valid, z)
    # conditions of the rows, on the restatement
    assert special <= 63 and not want_has[2] and not want_has[4] and want_z[2] == z[2] and want_has[[0, 1, 3, 5, 6, 7, 8, 9]].all()
    assert want_q[5] == 1 and z[5] == -1 and want_q[6] == -1 and z[6] == 1
    num, den = V.root_sums(N[9], Q[9], valid[9])
    assert f32(num / den) > 1 and want_q[9] == 1 and want_q[10] == -1
    assert int(N[7].astype(np.int64).sum()) > 1 << 24
    P = pkg()
    eng = P.Engine(2, blocks=1, sims=SIMS, dtype=P.NET_F32)
    for n in (1, 63, 64, 65, 130):
        q, has, zz = eng.debug_value_mix(q_share, N[:n], Q[:n], valid[:n], z[:n])
        assert q.tobytes() == want_q[:n].tobytes(), (n, q, want_q[:n])
        assert (has == want_has[:n]).all(), n
        assert zz.tobytes() == want_z[:n].tobytes(), (n, zz, want_z[:n])
    eng.close()
    if q_share == 1.0:
        assert (want_z[want_has] == want_q[want_has]).all()


# ---- 2. azr_mcts_root_value ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", [1, 2])
def test_root_value_is_the_restatement_on_root_stats(threads):
    eng = SR.engine(threads, SIMS)
    states, rngs = SR.late_positions()
    eng.set_states(states)
    eng.set_rng(rngs)
    eng.mcts_clear()
    q, has = eng.root_value()                                         # no root is in the tree yet
    assert not q.any() and not has.any()
    for step in range(3):                                             # three searches, a move between them: both players' roots
        eng.simulate()
        n, qq, _ = eng.root_stats()
        valid = eng.valid_moves()
        q, has = eng.root_value()
        want = [V.root_value(n[g], qq[g], valid[g]) for g in range(G)]
        assert q.tobytes() == np.array([w[0] for w in want], f32).tobytes(), (step, q, want)
        assert (has == np.array([w[1] for w in want])).all() and has.all()
        assert (eng.make_moves(eng.pick(sample=False)) == 0).all()
    eng.close()


# ---- 3. self-play is the host-stepped retrace with z' filled in by the restatement ---------------------------------------------------
def _run(threads, full, psw, on):
    """the four late games; `full`: under a playout cap, Dirichlet noise, forced playouts and pruning; psw: with surprise weighting;
    on = False: the setter is never called"""
    return SR.Run(BASE, QUOTA, threads, SIMS, surprise=(SHARE, MAXW, PSEED) if psw else None, value_mix=QSHARE if on else None,
                  **(dict(fast=FAST, cap=(0.5, CSEED), dirichlet=(ALPHA, NSEED), forced=(K, True)) if full else {}))


def _root_values(game):
    """(q [n], has_q [n]) by the restatement from azr_mcts_root_stats' N and Q at the game's recorded decisions"""
    qh = [V.root_value(n, qq, va) for n, qq, va in zip(game.N, game.Q, game.valid)]
    return np.array([x[0] for x in qh], f32), np.array([x[1] for x in qh], bool)


def _mixed(recs, z, q, has):
    """the retrace's records with z' by the restatement in bytes 89..92"""
    out = recs.copy()
    for r in range(len(out)):
        out[r, 89:93] = np.array([V.blend(z[r], q[r], has[r], QSHARE)], f32).view(np.uint8)
    return out


@pytest.mark.parametrize("threads,full,psw", [(1, False, False), (2, False, False), (2, True, False), (2, True, True)])
def test_selfplay_is_the_host_stepped_retrace_with_the_restated_blend(threads, full, psw):
    recs, c = SR.cached("selfplay", _run(threads, full, psw, True))
    games, tot = SR.cached("retrace", _run(threads, full, psw, True))
    roots = [_root_values(g) for g in games]
    z, q, has = np.concatenate([g.z for g in games]), np.concatenate([r[0] for r in roots]), np.concatenate([r[1] for r in roots])
    zz = np.array([V.blend(z[r], q[r], has[r], QSHARE) for r in range(len(z))], f32)
    print("records per game:", [len(g.records) for g in games], tot)
    print("z = +1: %d, z = -1: %d, q against z: %d, z' != z: %d, |z' - z| mean %.3f" %
          ((z == 1).sum(), (z == -1).sum(), (q * z < 0).sum(), (zz != z).sum(), float(np.abs(zz - z).mean())))
    # conditions of the test, on the retrace: both outcomes, a root value that disagrees with the outcome, a blend that moves z
    assert (z == 1).any() and (z == -1).any(), z
    assert (q * z < 0).any(), (q, z)
    assert (zz != z).any() and has.all()
    streams = []
    for g, (game, (gq, gh)) in enumerate(zip(games, roots)):
        copies = None
        if psw:
            kl = np.array([S.record_kl(pi, pr, va) for pi, pr, va in zip(pi_of(game.records), game.prior, game.valid)], f32)
            copies = S.game_copies(kl, SHARE, MAXW, PSEED, BASE + g)[1]
        streams.append((_mixed(game.records, game.z, gq, gh), copies))
    SR.assert_streams(recs, c, streams, tot)


# ---- 4. on against off ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads,full,psw", [(2, False, False), (2, True, True)])
def test_the_mix_changes_the_four_value_bytes_only(threads, full, psw):
    on, c1 = SR.cached("selfplay", _run(threads, full, psw, True))
    off, c0 = SR.cached("selfplay", _run(threads, full, psw, False))
    assert c0 == c1 and c0["samples"] == len(off) == len(on)
    mask = np.ones(265, bool); mask[89:93] = False

    def order(r):                                                   # (games that end in one pass may be flushed in either order)
        return r[np.lexsort(r[:, mask].T[::-1])]

    on, off = order(on), order(off)
    assert (on[:, mask] == off[:, mask]).all()
    z_off = off[:, 89:93].copy().view(f32)[:, 0]
    z_on = on[:, 89:93].copy().view(f32)[:, 0]
    assert set(z_off.tolist()) <= {-1.0, 0.0, 1.0}
    assert (z_on != z_off).any() and (np.abs(z_on) <= 1).all()


# ---- 5. slot independence ---------------------------------------------------------------------------------------------------------
def test_a_quota_writes_the_same_records_on_two_and_on_eight_slots():
    recs, _, _, samples = SR.quota_on_slots((2, 8), lambda eng: eng.selfplay_set_value_mix(QSHARE), SIMS, BASE)
    z = recs[:, 89:93].copy().view(f32)[:, 0]
    print("records %d, of them with a z' outside {-1, 0, 1}: %d" % (samples, int((~np.isin(z, [-1, 0, 1])).sum())))
    assert (~np.isin(z, [-1, 0, 1])).any()


# ---- 6. off is the engine that never called it ------------------------------------------------------------------------------------
def test_off_is_the_engine_that_never_called_it():
    def meddle(i, eng):
        if i == 0:                                                # on again while it runs
            assert eng.counters()["games_finished"] < QUOTA
            eng.selfplay_set_value_mix(QSHARE)

    def on_then_off(eng):                                         # on, then off before the start
        eng.selfplay_set_value_mix(QSHARE)
        eng.selfplay_set_value_mix(0.0)

    run = _run(2, False, False, False)
    never, c0 = SR.cached("selfplay", run)
    eng = SR.selfplay(run, on_then_off)
    recs, c = SR.play_out(eng, QUOTA, 16, 400, after_run=meddle)
    assert recs.tobytes() == never.tobytes() and c == c0
    # the next start reads the setting
    SR.place(eng, run)
    again, c = SR.play_out(eng, QUOTA, 16, 400)
    eng.close()
    on, c1 = SR.cached("selfplay", _run(2, False, False, True))
    assert on.tobytes() != never.tobytes()
    assert again.tobytes() == on.tobytes() and c == c1


# ---- 7. the arena never sees it ---------------------------------------------------------------------------------------------------
def test_the_arena_never_sees_it():
    P = pkg()
    eng = SR.engine(2, SIMS, 2, max_game_rounds=36)
    eng.selfplay_set_value_mix(QSHARE)
    res, _, recs, _ = arena_play(eng, P.PLAYER_ALPHAZERO, P.PLAYER_SCRIPT, 2, 0, False, BASE, az=True)
    eng.close()
    assert res["count"] == 2 and len(recs) > 0
    z = recs[:, 89:93].copy().view(f32)[:, 0]
    assert set(z.tolist()) <= {-1.0, 0.0, 1.0}, sorted(set(z.tolist()))


# ---- 8. argument errors -----------------------------------------------------------------------------------------------------------
def test_argument_errors():
    P = pkg()
    eng = P.Engine(2, blocks=1, sims=4, dtype=P.NET_F32, threads=2)
    L = eng.L
    assert L.azr_selfplay_set_value_mix(None, 0.5) == 3                         # AZR_E_BAD_HANDLE
    assert L.azr_mcts_root_value(None, None, None) == 3
    assert L.azr_debug_value_mix(None, 0.5, None, None, None, None, 0, None, None, None) == 3
    nan = float("nan")
    for bad in (nan, 1.5):
        with pytest.raises(P.AzrError) as e:
            eng.selfplay_set_value_mix(bad)
        assert e.value.code == 1 and "azr_selfplay_set_value_mix" in str(e.value), bad
    eng.selfplay_set_value_mix(0.0); eng.selfplay_set_value_mix(-2.0); eng.selfplay_set_value_mix(1.0); eng.selfplay_set_value_mix(0.0)
    N, Q, ok, z = np.full((1, 43), 2, np.uint32), np.full((1, 43), 0.5, f32), np.array([ALL], np.uint64), np.array([-1.0], f32)
    for bad in (0.0, -1.0, nan, 1.5):
        with pytest.raises(P.AzrError) as e:
            eng.debug_value_mix(bad, N, Q, ok, z)
        assert e.value.code == 1 and "azr_debug_value_mix" in str(e.value), bad
    assert L.azr_debug_value_mix(eng.h, 0.5, None, None, None, None, 1, None, None, None) == 1
    assert L.azr_mcts_root_value(eng.h, None, None) == 1
    q, has, zz = eng.debug_value_mix(0.5, N, Q, ok, z)
    assert q[0] == 0.5 and has[0] and zz[0] == -0.25
    eng.close()
