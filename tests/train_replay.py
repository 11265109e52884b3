"""The proof the optimiser-step tests share (TEST INFRASTRUCTURE, not collected): one engine is driven through a schedule of train,
validate, predict and reset calls (run_schedule), every recorded call is made again on a NEW engine that was given the weights of that
moment (replay), and the two must agree bit for bit (assert_pure): gradients and losses of a step are a function of the weights and the
minibatch alone — whatever the step before left in the training context (packed kernels, statistics slots, split-K slabs, the side
stream's events), whichever batch size or call came before.  What the replay cannot see — the Adam moments and the step count, which
a fresh engine does not have — adam_trajectory restates on the host across the whole schedule.  Nothing here compares with float64:
that is test_gpu_train.py::test_step_matches_torch_graph, on the first step of any weights.
epoch_loop_against_single_steps is the other proof two test files share: azr_nn_train's queue of steps against single train_batch calls.
An engine is anything with set_weights / get_weights / train_batch / train_grads / train_reset / validate / predict (and close); a
group of data-parallel ranks (tests/dp_group.py::DpGroup) is one, and adds solo_batch for the schedule kind "solo"."""
import os
import subprocess
from typing import NamedTuple, Optional, Tuple

import numpy as np

import torch_train_ref as train

f32 = np.float32
ADAM_BOUND = 5e-7    # per step on the trainable slots: a lost moment or a restarted step count moves weights by about the learning rate, 1e-3
E_STATE = 7          # AZR_E_STATE (include/azr.h): azr_nn_train_grads without a training context
TRAIN_KINDS = ("train", "solo")   # the schedule entries that take an optimiser step


class Step(NamedTuple):
    """one call of a schedule as it went on the engine under test (or, out of replay, on a fresh one).  w0 / w1: get_weights() before and
    after the call; rec: the 265-byte records the call was given (predict: their 88 input bytes); out: what the call returned —
    train: (loss_pi, loss_v), validate: (loss_pi, loss_v, per-record cross-entropy, per-record squared error), predict: (pi, v),
    reset: the error code train_grads() raised behind it (None: it returned a vector); grads: train_grads() behind a train step;
    fresh: no step has run on this engine since it was created or reset (m = v = 0, step count 0)"""
    kind: str
    bs: int
    w0: np.ndarray
    rec: Optional[np.ndarray]
    out: Tuple
    grads: Optional[np.ndarray]
    w1: np.ndarray
    fresh: bool


def kinds(blocks):
    """per AZRW slot: 1 = kernel (L2-regularised), 2 = BN gamma / beta and dense biases, 0 = BN moving statistics"""
    k = np.zeros(train.layout(blocks)[1], np.uint8)
    for name, off, shape in train.layout(blocks)[0]:
        n = int(np.prod(shape))
        if name.endswith("_bn"):
            k[off:off + 2 * shape[1]] = 2
        elif name.endswith("_b"):
            k[off:off + n] = 2
        else:
            k[off:off + n] = 1
    return k


def tf_adam(w, g, m, v, t, k):
    """tf.train.AdamOptimizer update in fp32 on the trainable slots; kernels get the L2 gradient 2e-3 w"""
    w, g, m, v = (a.astype(np.float32).copy() for a in (w, g, m, v))
    g = np.where(k == 1, g + np.float32(2e-3) * w, g)
    lr_t = np.float32(1e-3 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t))
    tr = k > 0
    m2 = np.float32(0.9) * m + np.float32(1 - 0.9) * g
    v2 = np.float32(0.999) * v + np.float32(1 - 0.999) * g * g
    w2 = w - lr_t * m2 / (np.sqrt(v2) + np.float32(1e-8))
    return np.where(tr, w2, w), np.where(tr, m2, m), np.where(tr, v2, v)


def _call(eng, kind, bs, rec):
    """the single call of one schedule step; returns (out, grads)"""
    if kind == "train":
        return tuple(eng.train_batch(rec)), eng.train_grads()
    if kind == "solo":      # a group of ranks (tests/dp_group.py): every rank takes the plain single-GPU step itself
        return tuple(eng.solo_batch(rec)), eng.train_grads()
    if kind == "validate":
        return tuple(eng.validate(rec, batch_size=bs, per_record=True)), None
    if kind == "predict":
        return tuple(eng.predict(rec)), None
    assert kind == "reset", kind
    eng.train_reset()
    try:
        eng.train_grads()
        return (None,), None
    except Exception as e:      # the binding's AzrError (or a fake's): what counts is the code
        return (getattr(e, "code", -1),), None


def run_schedule(make_engine, flat, schedule, rec):
    """drive ONE engine through the schedule — ("train", bs), ("solo", bs), ("validate", bs, nb), ("predict", n), ("reset",) — on
    consecutive, disjoint slices of rec; returns the trace, a Step per schedule entry.  "solo" is a train step too (TRAIN_KINDS)"""
    eng = make_engine()
    eng.set_weights(flat)
    trace, at, fresh = [], 0, True
    try:
        for s in schedule:
            kind, bs = s[0], (s[1] if len(s) > 1 else 0)
            n = bs * s[2] if kind == "validate" else bs
            assert at + n <= len(rec), "the schedule needs more records than it was given"
            r = rec[at:at + n].copy()
            at += n
            if kind == "predict":
                r = r[:, 1:89].copy()
            w0 = eng.get_weights()
            out, grads = _call(eng, kind, bs, r)
            trace.append(Step(kind, bs, w0, r if n else None, out, grads, eng.get_weights(), fresh))
            fresh = kind == "reset" or (fresh and kind not in TRAIN_KINDS)
    finally:
        if hasattr(eng, "close"):
            eng.close()
    return trace


def replay(make_engine, trace):
    """every recorded call again, each on an engine of its own that was given the weights from before the call; a Step per trace entry
    (None for a reset: there is nothing to repeat)"""
    out = []
    for s in trace:
        if s.kind == "reset":
            out.append(None)
            continue
        eng = make_engine()
        try:
            eng.set_weights(s.w0)
            o, grads = _call(eng, s.kind, s.bs, s.rec)
            out.append(Step(s.kind, s.bs, s.w0, s.rec, o, grads, eng.get_weights(), True))
        finally:
            if hasattr(eng, "close"):
                eng.close()
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint8)


def first_difference(a, b, layout):
    """(name of the first tensor of the layout in which the flat vectors a and b differ in a bit, differing entries in all) or None"""
    d = _bits(a) != _bits(b)
    if not d.any():
        return None
    for name, off, shape in layout:
        if d[off:off + int(np.prod(shape))].any():
            return name, int(d.sum())
    return "(outside the layout)", int(d.sum())


def _layout_of(count):
    for blocks in range(0, 64):
        lay, n = train.layout(blocks)
        if n == count:
            return lay
    raise AssertionError("no AZRW layout has %d parameters" % count)


def assert_pure(trace, replayed, layout=None, moving=None):
    """the engine under test did at every step what a fresh engine does with the same weights and inputs.
    train, solo: the loss pairs are ==, the gradient vectors equal as uint32 (neither the moving statistics' history nor the Adam state
              enter them); the moving statistics behind the step (slots where `moving` is set) are equal too: momentum 0.99 on the
              batch statistics, again weights and minibatch alone.  The trained slots behind the step are compared only where the
              step is `fresh` — the first one, and the first behind a reset: there the engine's m, v and step count are what the
              fresh engine's are, which is what azr_nn_train_reset promises — and then the WHOLE weight vector is equal as uint32.
    validate, predict: equal bytes, and the weights behind the call are the weights in front of it.
    reset:    weights untouched; azr_nn_train_grads then has no step to report and fails with AZR_E_STATE.
    layout: (name, offset, shape) rows naming the slots in the failure message (default: the AZRW layout of the vector's length);
    moving: boolean mask of the moving-statistics slots (default: kinds == 0 of that layout)"""
    assert len(trace) == len(replayed)
    if layout is None:
        layout = _layout_of(len(trace[0].w0))
    if moving is None:
        moving = np.ones(len(trace[0].w0), bool)
        for name, off, shape in layout:
            n = int(np.prod(shape))
            moving[off:off + (2 * shape[1] if name.endswith("_bn") else n)] = False
    for i, (a, b) in enumerate(zip(trace, replayed)):
        where = "step %d (%s, batch %d)" % (i, a.kind, a.bs)
        if a.kind == "reset":
            assert first_difference(a.w0, a.w1, layout) is None, "%s: the reset changed the weights: %s" % (where, first_difference(a.w0, a.w1, layout))
            assert a.out == (E_STATE,), "%s: train_grads behind a reset must fail with AZR_E_STATE, got %r" % (where, a.out)
            continue
        assert b is not None and first_difference(a.w0, b.w0, layout) is None, where
        if a.kind in TRAIN_KINDS:
            assert a.out == b.out, "%s: losses %r, on a fresh engine %r" % (where, a.out, b.out)
            d = first_difference(a.grads, b.grads, layout)
            assert d is None, "%s: gradients differ from a fresh engine's, first in %s, %d entries in all" % ((where,) + d)
            d = first_difference(np.where(moving, a.w1, 0), np.where(moving, b.w1, 0), layout)
            assert d is None, "%s: moving statistics differ from a fresh engine's, first in %s, %d entries in all" % ((where,) + d)
            if a.fresh:
                d = first_difference(a.w1, b.w1, layout)
                assert d is None, "%s: first step on cleared optimiser state, weights differ from a fresh engine's, first in %s, %d entries in all" % ((where,) + d)
            continue
        for k, (x, y) in enumerate(zip(a.out, b.out)):
            x, y = np.asarray(x), np.asarray(y)
            same = x.shape == y.shape and x.tobytes() == y.tobytes()
            assert same, "%s: output %d differs from a fresh engine's in %d entries" % (
                where, k, int((_bits(x.astype(f32)) != _bits(y.astype(f32))).sum()) if x.shape == y.shape else -1)
        d = first_difference(a.w0, a.w1, layout)
        assert d is None, "%s: the call changed the weights, first in %s, %d entries in all" % ((where,) + d)


def adam_trajectory(trace, kinds):
    """tf_adam on the engine's own gradients, step by step over the whole schedule: m, v and the step count t are carried HERE — across
    every context rebuild and every validate / predict in between — and cleared at a reset; w starts every step from the engine's
    weights (no drift adds up).  Every train step must land within ADAM_BOUND of it on the trainable slots.  Returns the worst deviation."""
    n = len(trace[0].w0)
    m, v, t = np.zeros(n, f32), np.zeros(n, f32), 0
    tr = kinds > 0
    worst = 0.0
    for i, s in enumerate(trace):
        if s.kind == "reset":
            m, v, t = np.zeros(n, f32), np.zeros(n, f32), 0
        if s.kind not in TRAIN_KINDS:
            continue
        t += 1
        w, m, v = tf_adam(s.w0, s.grads, m, v, t, kinds)
        dev = float(np.abs(s.w1[tr] - w[tr]).max())
        assert dev <= ADAM_BOUND, "step %d (%s, batch %d), Adam step %d: weights %.3g away from Adam on the carried moments" % (i, s.kind, s.bs, t, dev)
        worst = max(worst, dev)
    return worst


def epoch_loop_against_single_steps(P, tmp_path, blocks, bs, n, epochs, state, flat, rec):
    """azr_nn_train over `epochs` epochs of n records (floor(n / bs) steps each, queued back to back, the remainder dropped) against
    train_batch driven by libstdc++'s own std::shuffle on minstd_rand0 (tests/helpers/shuffle_probe.cpp): equal epoch-average losses,
    weights equal as uint32.  Returns (the engine that ran the loop, still open; the shuffle state it handed back; the probe's)."""
    exe = str(tmp_path / "shuffle_probe")
    subprocess.check_call(["g++", "-O1", "-o", exe, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "shuffle_probe.cpp")])
    out = subprocess.check_output([exe, str(n), str(state), str(epochs)]).decode().split("\n")
    perms = [np.array(out[e].split(), int) for e in range(epochs)]
    end_state = int(out[epochs])
    a = P.Engine(8, blocks=blocks, sims=1, dtype=P.NET_F32, node_capacity=64)
    a.set_weights(flat)
    hist, st = a.train(rec, epochs, batch_size=bs, rng_state=state)
    b = P.Engine(8, blocks=blocks, sims=1, dtype=P.NET_F32, node_capacity=64)
    b.set_weights(flat)
    for e in range(epochs):
        lp = lv = np.float32(0)
        for c in range(n // bs):
            l = b.train_batch(rec[perms[e][c * bs:(c + 1) * bs]])
            lp += np.float32(l[0]); lv += np.float32(l[1])
        assert hist[e] == (float(lp / np.float32(n // bs)), float(lv / np.float32(n // bs))), (e, hist[e])
    assert (a.get_weights().view(np.uint32) == b.get_weights().view(np.uint32)).all()
    b.close()
    return a, st, end_state
