"""CPU: tests/golden/scripted_samples.npz — the records the reference's ScriptPlayer / RandomPlayer push into a train
storage attached to both players (Player::addTrainingSample, player/base/player.cpp:9-17), the fixture the device's
scripted collection is pinned to (tests/test_gpu_scripted_samples.py)."""
import importlib.util
import os

import numpy as np
import pytest

import azr_testlib as T

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "scripted_samples.npz")


def _gen():
    spec = importlib.util.spec_from_file_location("make_scripted_samples_golden",
                                                  os.path.join(HERE, "golden", "make_scripted_samples_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _records_of(full):
    pi = full[:, 93:265].copy().view(np.float32)
    z = full[:, 89:93].copy().view(np.float32)[:, 0]
    return full[:, 0], pi, z


@pytest.mark.ref
@pytest.mark.skipif(not T.have_ref() or not os.path.isdir(os.path.join(_gen().REF, "src")),
                    reason="oracle/_ref or the reference's sources are absent")
def test_probe_rebuilds_the_fixture_bit_for_bit():
    new = _gen().generate()
    old = np.load(FIX)
    assert sorted(new) == sorted(old.files)
    for k in old.files:
        assert new[k].dtype == old[k].dtype and np.array_equal(new[k], old[k]), k


def test_fixture_records_are_one_hot_with_the_game_value():
    f = np.load(FIX)
    assert f["count"].min() > 0 and len(f["digest"]) == f["count"].sum()
    assert len(np.unique(f["digest"])) == len(f["digest"])   # every record differs: a digest identifies it
    for key in ("11", "12", "21"):
        player, pi, z = _records_of(f["full_" + key])
        c, g, i = f["full_at_" + key]
        status = int(f["status"][c, g, i])
        assert len(player) == f["count"][c, g, i]
        assert ((pi == 1.0).sum(1) == 1).all() and ((pi != 0.0).sum(1) == 1).all()
        assert (np.argmax(pi, 1) <= 42).all()
        assert set(np.unique(z)) <= {-1.0, 0.0, 1.0}
        expect = np.where(status == 2, 0.0, np.where(player == status, 1.0, -1.0)).astype(np.float32)   # DRAW = 2
        assert (z == expect).all(), key
        assert set(np.unique(player)) == {0, 1} or key != "11"


def test_fixture_games_are_the_arena_games_of_the_oracle():
    """recording changed no play on the reference side: each slot's statuses and round counts are those of the same slot
    without a storage (the oracle, pinned to ref_play_games by tests/test_oracle_vs_ref.py)"""
    f = np.load(FIX)
    for c, (k0, k1, mirror, base) in enumerate(f["configs"]):
        for g in range(f["count"].shape[1]):
            games = f["count"].shape[2]
            _, st, rd, _, _ = T.orc_play_games(int(k0), int(k1), games, bool(mirror), int(base) + g)
            assert (f["status"][c, g] == st).all() and (f["rounds"][c, g] == rd).all(), (c, g)
