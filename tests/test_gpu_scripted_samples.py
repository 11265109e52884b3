"""GPU: scripted collection (azr_arena_collect_scripted_samples) — ScriptPlayer / RandomPlayer record one-hot samples at the
reference's addTrainingSample sites (player/base/player.cpp:9-17), the seam of `-m train-data` / `-m train-script`.
Pinned record for record to the reference (tests/golden/scripted_samples.npz), with the ring-room contract: nothing dropped,
a run returns unfinished only to wait for a drain."""
import hashlib
import os

import numpy as np
import pytest

import azr_testlib as T
from gpu_common import arena_play as play, assert_one_hot, pi_of, pkg

pytestmark = pytest.mark.gpu
FM = T.data_field_mask()
FIX = os.path.join(T.GOLDEN, "scripted_samples.npz")


def digests(rec):
    return np.array([np.frombuffer(hashlib.blake2b(r.tobytes(), digest_size=8).digest(), np.uint64)[0] for r in rec], np.uint64)


def z_of(rec):
    return rec[:, 89:93].copy().view(np.float32)[:, 0]


def game_blocks(rec):
    """a ring of whole games, each one contiguous block in move order: split where the round (bytes 45..46) goes down"""
    rnd = rec[:, 45].astype(np.int32) | (rec[:, 46].astype(np.int32) << 8)
    cut = [0] + [i for i in range(1, len(rec)) if rnd[i] < rnd[i - 1]] + [len(rec)]
    return [rec[a:b] for a, b in zip(cut[:-1], cut[1:])]


@pytest.mark.parametrize("c", range(6))
def test_scripted_records_equal_the_reference_fixture(c):
    """G = 3, 4 games per slot, the fixture's seeds: every drained game is one fixture game, record for record (digests);
    every fixture game is met exactly once"""
    P = pkg()
    f = np.load(FIX)
    k0, k1, mirror, base = (int(v) for v in f["configs"][c])
    cnt = f["count"]
    first = int(cnt[:c].sum())
    games = {}   # digest of a game's first record -> (slot, game, offset into the fixture's digests)
    at = first
    for g in range(cnt.shape[1]):
        for i in range(cnt.shape[2]):
            d = int(f["digest"][at])
            assert d not in games   # every deal differs
            games[d] = (g, i, at)
            at += int(cnt[c, g, i])
    eng = P.Engine(3, blocks=1, sims=1, dtype=P.NET_F32, node_capacity=64)
    res, (n, st, rd, _), rec, _ = play(eng, k0, k1, 10 ** 6, 4, P.MIRROR_SEQUENTIAL if mirror else False, base, script=True)
    assert (n == 4).all() and eng.counters()["errors"] == 0 and eng.counters()["records_dropped"] == 0
    assert (st[:, :4] == f["status"][c]).all() and (rd[:, :4] == f["rounds"][c]).all()
    dg = digests(rec)
    assert len(dg) == int(cnt[c].sum())
    p, seen = 0, set()
    while p < len(dg):
        key = int(dg[p])
        assert key in games and key not in seen, p
        seen.add(key)
        g, i, off = games[key]
        k = int(cnt[c, g, i])
        assert (dg[p:p + k] == f["digest"][off:off + k]).all(), (g, i)
        p += k
    assert len(seen) == len(games)
    assert eng.counters()["samples"] == len(rec)
    eng.close()


def test_recording_does_not_change_play():
    """1024 slots x 10 RandomPlayer vs ScriptPlayer games, unmirrored (test_gpu_arena's ten-thousand-games setting): with
    scripted collection on, results, statuses, rounds and finals are those of the run without it"""
    P = pkg()
    G, per_slot, base = 1024, 10, 900000
    eng = P.Engine(G, blocks=1, sims=1, dtype=P.NET_F32, node_capacity=64)
    res0, (n0, st0, rd0, fin0), _, _ = play(eng, P.PLAYER_RANDOM, P.PLAYER_SCRIPT, 10 ** 7, per_slot, False, base)
    seen = [0]

    def check(rec):
        assert_one_hot(rec)
        assert set(np.unique(z_of(rec))) <= {-1.0, 0.0, 1.0}
        seen[0] += len(rec)

    res1, (n1, st1, rd1, fin1), _, _ = play(eng, P.PLAYER_RANDOM, P.PLAYER_SCRIPT, 10 ** 7, per_slot, False, base, script=True,
                                            chunk=1 << 18, sink=check)
    cn = eng.counters()
    assert res1 == res0 and (n1 == n0).all() and (n1 == per_slot).all()
    assert (st1 == st0).all() and (rd1 == rd0).all() and (fin1[..., FM] == fin0[..., FM]).all()
    assert cn["errors"] == 0 and cn["records_dropped"] == 0 and cn["samples"] == seen[0] > 0
    eng.close()


@pytest.mark.parametrize("mirror", ["sequential", "concurrent"])
def test_ring_room_contract_nothing_dropped(mirror):
    """G = 64, sample_capacity 2048 (a ring of 131 072 records), 1280 Script-vs-Script games (~380 k records): several
    run / drain rounds, no record dropped, the same records as an engine whose ring holds them all, the same results as
    the run without collection"""
    P = pkg()
    G, per_slot, base = 64, 20, 31000
    m = P.MIRROR_SEQUENTIAL if mirror == "sequential" else P.MIRROR_CONCURRENT
    cap = per_slot if m == P.MIRROR_SEQUENTIAL else 0
    total = G * per_slot
    small = P.Engine(G, blocks=1, sims=1, dtype=P.NET_F32, node_capacity=64, sample_capacity=2048)
    res0, (n0, st0, rd0, _), _, _ = play(small, P.PLAYER_SCRIPT, P.PLAYER_SCRIPT, total, cap, m, base)
    res1, (n1, st1, rd1, _), rec, waits = play(small, P.PLAYER_SCRIPT, P.PLAYER_SCRIPT, total, cap, m, base, script=True)
    cn = small.counters()
    small.close()
    assert waits >= 2, waits   # the ring of 131 k records had to be drained at least twice on the way
    assert cn["records_dropped"] == 0 and cn["errors"] == 0 and cn["samples"] == len(rec)
    assert res1 == res0 and res1["count"] == total and (n1 == n0).all() and (st1 == st0).all() and (rd1 == rd0).all()
    big = P.Engine(G, blocks=1, sims=1, dtype=P.NET_F32, node_capacity=64, sample_capacity=16384)
    _, _, ref, waits_big = play(big, P.PLAYER_SCRIPT, P.PLAYER_SCRIPT, total, cap, m, base, script=True)
    assert big.counters()["records_dropped"] == 0
    big.close()
    assert waits_big == 0 and len(ref) == len(rec) > 2 * G * 2048
    assert (np.sort(digests(rec)) == np.sort(digests(ref))).all()
    assert_one_hot(rec)


@pytest.mark.parametrize("az_first", [True, False])
def test_alphazero_vs_script_both_collections(orc, az_first):
    """AlphaZero vs ScriptPlayer (configs[0] shape, small f32 net): with both collections on, the AlphaZero side's records of a
    game are byte for byte those of azr_arena_collect_samples alone (pinned to the oracle by test_gpu_arena), the Script
    side's are one-hot with the opposite z, and scripted collection alone yields exactly the Script side's"""
    P = pkg()
    G, per_slot, S, B, base = 6, 2, 16, 1, 4100
    eng = P.Engine(G, blocks=B, sims=S, dtype=P.NET_F32)
    eng.set_weights(T.make_net_flat(B, seed=21, perturb_bn=True))
    k = (P.PLAYER_ALPHAZERO, P.PLAYER_SCRIPT) if az_first else (P.PLAYER_SCRIPT, P.PLAYER_ALPHAZERO)
    az_p = 0 if az_first else 1
    res_a, log_a, rec_a, _ = play(eng, k[0], k[1], 10 ** 6, per_slot, True, base, az=True)
    res_b, log_b, rec_b, _ = play(eng, k[0], k[1], 10 ** 6, per_slot, True, base, az=True, script=True)
    res_c, log_c, rec_c, _ = play(eng, k[0], k[1], 10 ** 6, per_slot, True, base, script=True)
    assert eng.counters()["errors"] == 0 and eng.counters()["records_dropped"] == 0
    assert res_a == res_b == res_c and (log_a[1] == log_b[1]).all() and (log_a[1] == log_c[1]).all()
    both = game_blocks(rec_b)
    assert len(both) == G * per_slot
    az_parts = sorted(b[b[:, 0] == az_p].tobytes() for b in both)
    sc_parts = sorted(b[b[:, 0] != az_p].tobytes() for b in both)
    assert az_parts == sorted(b.tobytes() for b in game_blocks(rec_a))
    assert sc_parts == sorted(b.tobytes() for b in game_blocks(rec_c))
    for b in both:
        a, s = b[b[:, 0] == az_p], b[b[:, 0] != az_p]
        assert len(a) and len(s)
        assert_one_hot(s)
        assert ((pi_of(a) != 0).sum(1) > 1).any()   # the search's visit distributions
        za, zs = np.unique(z_of(a)), np.unique(z_of(s))
        assert len(za) == 1 and len(zs) == 1 and zs[0] == -za[0]
    eng.close()
