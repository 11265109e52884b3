"""GPU: device-resident self-play on a sharp net (azr_testlib.make_sharp_net_flat(1, seed=11): priors of exactly 0 and 1 with the
peak often on an illegal move, denormal priors, values of exactly +-1) — the outputs of a trained net, which the random-init nets of
the other self-play tests never give.  The same comparisons as theirs, through the same harness (tests/selfplay_retrace.py with
Run.net = "sharp"): the four late golden games in device self-play against their host-stepped retrace, bit for bit and record by
record, plain and with Dirichlet noise, forced playouts with pruning, a playout cap, surprise weighting and the value mix (each with
its own restatement: surprise_ref, value_mix_ref), under the Gumbel root search and its tree selection (tests/gumbel_retrace.py); whole
games from the start against the oracle's orc_selfplay_game with the device net called back; and the two-net arena of sharp nets
against the oracle.  Resignation on this net is in tests/test_gpu_resign.py, beside the assertion it reuses.
Every run ends with errors == 0, nodes_dropped == 0 and records_dropped == 0 at the default node capacity."""
import numpy as np
import pytest

import azr_testlib as T
import gumbel_retrace as GR
import selfplay_retrace as SR
import surprise_ref as S
import value_mix_ref as V
from gpu_common import concurrent_two_net_arena, pi_of, selfplay_games

pytestmark = pytest.mark.gpu

f32 = np.float32
BASE, NSEED, CSEED, SIMS, FAST, ALPHA, K, QUOTA = 9100, 77, 99, 8, 4, 0.3, 2.0, 4
SHARE, MAXW, PSEED = 0.75, 4.0, 31
QSHARE = 0.5

OPTIONS = {
    "plain": {},
    "dirichlet": dict(dirichlet=(ALPHA, NSEED)),
    "forced_pruned": dict(forced=(K, True)),
    "playout_cap": dict(fast=FAST, cap=(0.5, CSEED)),
    "surprise": dict(surprise=(SHARE, MAXW, PSEED)),
    "value_mix": dict(value_mix=QSHARE),
    "all": dict(fast=FAST, cap=(0.5, CSEED), dirichlet=(ALPHA, NSEED), forced=(K, True), surprise=(SHARE, MAXW, PSEED), value_mix=QSHARE),
}


def _mixed(game):
    """the retrace's records with z' by the restatement in bytes 89..92"""
    out = game.records.copy()
    for r in range(len(out)):
        q, has = V.root_value(game.N[r], game.Q[r], game.valid[r])
        out[r, 89:93] = np.array([V.blend(game.z[r], q, has, QSHARE)], f32).view(np.uint8)
    return out


@pytest.mark.parametrize("threads", [1, 2])
@pytest.mark.parametrize("option", list(OPTIONS))
def test_sharp_selfplay_is_the_host_stepped_retrace(option, threads):
    run = SR.Run(BASE, QUOTA, threads, SIMS, net="sharp", **OPTIONS[option])
    recs, c = SR.cached("selfplay", run)       # play_out asserts errors == 0, nodes_dropped == 0, records_dropped == 0
    games, tot = SR.cached("retrace", run)
    prior = np.concatenate([g.prior for g in games])
    q = np.concatenate([g.Q for g in games])
    n = np.concatenate([g.N for g in games])
    pi = np.concatenate([pi_of(g.records) for g in games])
    print("%s T=%d: %d records; roots with a zero legal prior row %d, a denormal prior %d, a visited |Q| == 1 %d, a one-hot policy %d" % (
        option, threads, len(prior), (prior == 0).all(1).sum(), ((prior > 0) & (prior < T.FLT_MIN)).any(1).sum(),
        ((n > 0) & (np.abs(q) == 1)).any(1).sum(), (pi == 1).any(1).sum()))
    # the regime, on the retrace: the net's zeros and its saturated values reach the roots of these games
    assert (prior == 0).all(1).any() and ((n > 0) & (np.abs(q) == 1)).any()
    streams = []
    for g, game in enumerate(games):
        copies = None
        if run.surprise:
            kl = np.array([S.record_kl(p, pr, va) for p, pr, va in zip(pi_of(game.records), game.prior, game.valid)], f32)
            assert np.isfinite(kl).all()
            copies = S.game_copies(kl, SHARE, MAXW, PSEED, BASE + g)[1]
        streams.append((_mixed(game) if run.value_mix is not None else game.records, copies))
    SR.assert_streams(recs, c, streams, tot)


@pytest.mark.parametrize("threads", [1, 2])
@pytest.mark.parametrize("tree", [0, 1], ids=["gumbel", "gumbel_tree"])
def test_sharp_gumbel_selfplay_is_the_host_stepped_retrace(tree, threads):
    """the Gumbel root search (m = 4, 16 simulations), and with the improved-policy selection below the root, through
    tests/gumbel_retrace.py: logits of zero priors at the FLT_MIN clamp, completed Q from values of +-1"""
    run = SR.Run(BASE, QUOTA, threads, 16, net="sharp")
    recs, c, rng_dev = GR.selfplay(run, 4, tree)
    games, tot, rng_ref = GR.retrace(run, 4, tree)
    prior = np.concatenate([g.prior for g in games])
    print("tree %d T=%d: %d records; roots with a zero legal prior row %d, a denormal prior %d" % (
        tree, threads, len(prior), (prior == 0).all(1).sum(), ((prior > 0) & (prior < T.FLT_MIN)).any(1).sum()))
    assert (prior == 0).all(1).any()
    SR.assert_streams(recs, c, [(g.records, None) for g in games], tot)
    assert rng_dev == rng_ref, (rng_dev, rng_ref)            # no rFloat: the dice streams after the last move
    pi = pi_of(recs)
    assert np.isfinite(pi).all() and np.abs(pi.astype(np.float64).sum(1) - 1).max() <= 43 * 2.0 ** -24


def test_sharp_two_net_arena_vs_oracle(orc):
    """sharp seeds 31 against 32 in concurrent mirrored pairs: results, final states, rounds and every collected record against the
    oracle's slots with the two device nets called back — the comparison of tests/test_gpu_arena.py.  Four games of 28 rounds (two turns
    past the set-up phase): sixteen games of 30 rounds pass alike and take 22 s, nearly all of it the oracle's calls back into the net."""
    c = concurrent_two_net_arena(orc, 2, False, T.make_sharp_net_flat(1, seed=31), T.make_sharp_net_flat(1, seed=32), G=2, S=8, rounds=28,
                                 dtype_name="NET_F32")
    assert c["errors"] == 0 and c["nodes_dropped"] == 0 and c["records_dropped"] == 0, c


@pytest.mark.parametrize("threads", [1, 2])
def test_sharp_whole_games_vs_oracle(orc, threads):
    """two games from the start (6 simulations, 12 rounds) against orc_selfplay_game with the device's sharp net called back"""
    c = selfplay_games(orc, threads, G=2, flat=T.make_sharp_net_flat(1, seed=11), max_game_rounds=12)
    assert c["errors"] == 0 and c["nodes_dropped"] == 0 and c["records_dropped"] == 0, c
