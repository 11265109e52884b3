"""GPU: the optimiser state lives apart from the batch-sized slabs (csrc/azr_train.hip: TrainState / Slabs).  A call with another batch
size rebuilds the slabs and nothing else; a rebuild that fails half-way (test hook AZR_TRAIN_FAIL_ALLOC=k in libazr_hip_test.so: the
k-th slab allocation returns AZR_E_HIP from the host, before hipMalloc and before any launch) leaves the handle with its state and no
slabs, and the next call builds them.  Every call here either succeeds or returns from the host: the device is never asked to misbehave.
Engine: 8 games, NET_F32, B = 1; ema_decay 0.75 and clip_norm 1, so the statistics row, the EMA vector and both update kernels are in
play.  A step is a pure function of state and minibatch (tests/test_gpu_train_replay.py), so a twin engine that never saw a failure
supplies the expected bits."""
import functools
import os

import numpy as np
import pytest

import azr_testlib as T
from gpu_common import pkg, records

pytestmark = pytest.mark.gpu

E_HIP = 4
HOOK = "AZR_TRAIN_FAIL_ALLOC"
# slabs_ensure allocates X0 col0 Y A G DS DT dY part wpart ap[0..2] dyp[0] dyp2[0] dyp[1] dyp2[1] af[0..1] pv0 dpv fpi fv h1 vout prob lossb hpart
# cpart in88 pit zt: 32 calls.  The first, two in the middle (DT, lossb) and the last
N_SLABS = 32
FAIL_AT = (1, 7, 27, N_SLABS)
OPTS = dict(ema_decay=0.75, clip_norm=1.0)


@functools.lru_cache(maxsize=None)
def _rec():
    return records(160, seed=41)


def _engine():
    P = pkg()
    e = P.Engine(8, blocks=1, sims=1, dtype=P.NET_F32, node_capacity=64, test_hooks=True)
    e.set_weights(T.make_net_flat(1, seed=11, perturb_bn=True))
    e.train_set_options(**OPTS)
    return e


def _snap(e):
    """weights, gradients, EMA vector and stats of the handle, as bytes"""
    st = e.train_stats()
    return (e.get_weights().tobytes(), e.train_grads().tobytes(), e.get_ema_weights().tobytes(),
            np.array([st[k] for k in sorted(st)], np.float64).tobytes())


def _call(e, call):
    kind, lo, n = call
    if kind == "train":
        e.train_batch(_rec()[lo:lo + n])
    else:
        e.validate(_rec()[lo:lo + n], batch_size=n)


TRAIN_18 = (("train", 0, 16), ("train", 16, 18), ("train", 34, 16))
VALIDATE_48 = (("train", 0, 16), ("validate", 50, 48), ("train", 34, 16))


@functools.lru_cache(maxsize=None)
def _twin(calls):
    """the snapshots behind every training call of an engine on which no allocation failed; computed once per sequence"""
    assert HOOK not in os.environ
    e = _engine()
    out = []
    for c in calls:
        _call(e, c)
        if c[0] == "train":
            out.append(_snap(e))
    e.close()
    return out


def _fails_twice(e, call, before):
    """with the hook set the call fails, and fails again (no batch size without its buffers passes the check); the state stays `before`"""
    P = pkg()
    for _ in range(2):
        with pytest.raises(P.AzrError) as ei:
            _call(e, call)
        assert ei.value.code == E_HIP and "injected" in str(ei.value)
        assert _snap(e) == before


@pytest.mark.parametrize("k", FAIL_AT)
def test_a_failed_rebuild_costs_nothing(k, monkeypatch):
    monkeypatch.delenv(HOOK, raising=False)
    tw = _twin(TRAIN_18)
    e = _engine()
    _call(e, TRAIN_18[0])
    before = _snap(e)
    assert before == tw[0]
    monkeypatch.setenv(HOOK, str(k))
    _fails_twice(e, TRAIN_18[1], before)
    monkeypatch.delenv(HOOK)
    _call(e, TRAIN_18[1])
    assert _snap(e) == tw[1]
    _call(e, TRAIN_18[2])
    assert _snap(e) == tw[2]
    e.close()


@pytest.mark.parametrize("k", FAIL_AT)
def test_a_failed_rebuild_inside_validate_costs_nothing(k, monkeypatch):
    monkeypatch.delenv(HOOK, raising=False)
    tw = _twin(VALIDATE_48)
    e = _engine()
    _call(e, VALIDATE_48[0])
    before = _snap(e)
    assert before == tw[0]
    monkeypatch.setenv(HOOK, str(k))
    _fails_twice(e, VALIDATE_48[1], before)
    monkeypatch.delenv(HOOK)
    _call(e, VALIDATE_48[2])     # the twin validated in between: a validation pass leaves no trace
    assert _snap(e) == tw[1]
    e.close()


def test_the_hook_counts_the_slab_allocations(monkeypatch):
    """N_SLABS is the last one: an index behind it is never reached, the rebuild succeeds"""
    monkeypatch.setenv(HOOK, str(N_SLABS + 1))
    e = _engine()
    _call(e, TRAIN_18[0])
    _call(e, TRAIN_18[1])
    e.close()


def test_gradients_survive_a_rebuild(monkeypatch):
    """azr_nn_train_grads is the last STEP's vector, whatever was rebuilt since"""
    monkeypatch.delenv(HOOK, raising=False)
    e = _engine()
    _call(e, VALIDATE_48[0])
    before = _snap(e)
    assert np.frombuffer(before[1], np.uint32).any()
    _call(e, VALIDATE_48[1])
    assert _snap(e) == before
    e.close()
