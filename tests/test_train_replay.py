"""CPU: the checks of tests/train_replay.py on a made-up engine (numpy only), so that the proof the optimiser-step tests share cannot
pass when it should not: the honest engine is accepted, assert_pure refuses every way a step can depend on more than its weights and
minibatch, adam_trajectory every way the optimiser state can get lost."""
import numpy as np
import pytest

import train_replay as TR

f32 = np.float32
# a layout in the AZRW style: kernels, batch norms (gamma, beta | moving mean, moving variance), a dense bias
LAYOUT = [("a_w", 0, (3, 8)), ("a_bn", 24, (4, 5)), ("b_w", 44, (16,)), ("b_b", 60, (4,))]
COUNT = 64
KINDS = np.zeros(COUNT, np.uint8)
KINDS[0:24] = 1; KINDS[24:34] = 2; KINDS[44:60] = 1; KINDS[60:64] = 2
SCHEDULE = [("train", 6), ("train", 6), ("validate", 6, 2), ("train", 6), ("train", 10), ("validate", 4, 1), ("train", 10),
            ("predict", 3), ("train", 4), ("reset",), ("train", 4), ("train", 6)]


class FakeError(RuntimeError):
    def __init__(self, code):
        super().__init__("fake error %d" % code)
        self.code = code


class Fake:
    """an engine whose "gradient" is a deterministic function of weights and records; a training context per batch size as the product
    has one (created by train_batch and validate, dropped by train_reset), Adam by TR.tf_adam.  spoil names the one defect it has."""

    def __init__(self, spoil=None):
        self.spoil = spoil
        self.ctx_bs = None            # the training context: batch size it was built for, Adam state, last gradients
        self.m = self.v = self.g = None
        self.t = 0
        self.steps = 0                # train steps of this engine's life
        self.packed = None            # what a stale pack would still hold
        self.validated = False
        self.prev_bs = None
        self.kept = False             # a reset that left the moments and the step count behind

    def set_weights(self, w):
        self.w = np.array(w, f32)
        self.w_infer = self.w.copy()

    def get_weights(self):
        return self.w.copy()

    def _ensure(self, bs):
        if self.ctx_bs == bs:
            return
        if self.ctx_bs is None and not self.kept:
            self.m, self.v, self.t = np.zeros(COUNT, f32), np.zeros(COUNT, f32), 0
        elif self.spoil == "m zeroed by a rebuild":
            self.m = np.zeros(COUNT, f32)
        elif self.spoil == "t restarts at a rebuild":
            self.t = 0
        self.kept = False
        self.ctx_bs, self.g = bs, np.zeros(COUNT, f32)

    @staticmethod
    def _feat(rec):
        return np.resize(np.asarray(rec, f32).mean(0) / f32(255), COUNT).astype(f32)

    def _grad(self, w, rec):
        g = (np.tanh(w) * f32(0.25) + self._feat(rec) - f32(0.4)).astype(f32)
        return np.where(KINDS > 0, g, f32(0))

    def train_batch(self, rec):
        bs = len(rec)
        self._ensure(bs)
        self.steps += 1
        w_used = self.packed if (self.spoil == "stale pack" and self.packed is not None) else self.w
        g = self._grad(w_used, rec)
        self.packed = self.w.copy()
        loss = (float(f32(g.sum())), float(f32((g * g).sum())))
        if self.spoil == "validate leaves a trace" and self.validated:
            g[3] += f32(1e-3)
        if self.spoil == "previous batch size" and self.prev_bs not in (None, bs):
            g[50] *= f32(1.5)
        if self.spoil == "bit flip at step 3" and self.steps == 3:
            g[61:62].view(np.uint32)[0] ^= 1
        self.prev_bs = bs
        if self.spoil == "loss last bit" and self.steps >= 2:
            loss = (float(np.nextafter(f32(loss[0]), f32(np.inf))), loss[1])
        self.t += 1
        before = self.w.copy()
        w, self.m, self.v = TR.tf_adam(self.w, g, self.m, self.v, self.t, KINDS)
        mov = KINDS == 0
        w[mov] = (f32(0.99) * self.w + f32(0.01) * self._feat(rec))[mov]
        self.w, self.g = w.astype(f32), g
        self.w_infer = before if self.spoil == "stale inference image" else self.w.copy()
        return loss

    def train_grads(self):
        if self.ctx_bs is None:
            raise FakeError(TR.E_STATE)
        return self.g.copy()

    def train_reset(self):
        self.kept = self.spoil == "m, v kept through reset" and self.ctx_bs is not None
        self.ctx_bs = None

    def validate(self, rec, batch_size, per_record):
        assert per_record and len(rec) % batch_size == 0
        self._ensure(batch_size)
        self.validated = True
        r = np.asarray(rec, f32) @ np.resize(self.w, rec.shape[1])
        return float(f32(r.mean())), float(f32((r * r).mean())), r.astype(f32), (r * r).astype(f32)

    def predict(self, x):
        p = (np.asarray(x, f32) @ np.resize(self.w_infer, (x.shape[1], 5))).astype(f32)
        return p, p.sum(1).astype(f32)


def _run(spoil):
    rng = np.random.default_rng(3)
    flat = rng.normal(0, 0.5, COUNT).astype(f32)
    rec = rng.integers(0, 256, (120, 265)).astype(np.uint8)
    make = lambda: Fake(spoil)
    trace = TR.run_schedule(make, flat, SCHEDULE, rec)
    return trace, TR.replay(make, trace)


def _moving():
    return KINDS == 0


def test_the_honest_engine_passes():
    trace, replayed = _run(None)
    assert [s.kind for s in trace] == [s[0] for s in SCHEDULE] and replayed[9] is None
    assert [s.fresh for s in trace if s.kind == "train"] == [True, False, False, False, False, False, True, False]
    # disjoint, consecutive slices of the records
    assert sum(len(s.rec) for s in trace if s.rec is not None) == 6 + 6 + 12 + 6 + 10 + 4 + 10 + 3 + 4 + 4 + 6
    TR.assert_pure(trace, replayed, LAYOUT, _moving())
    worst = TR.adam_trajectory(trace, KINDS)
    assert worst <= TR.ADAM_BOUND
    assert max(np.abs(s.w1 - s.w0)[KINDS > 0].max() for s in trace if s.kind == "train") > 1e-4   # the steps do move the weights


@pytest.mark.parametrize("spoil", ["stale pack", "validate leaves a trace", "previous batch size", "bit flip at step 3", "loss last bit",
                                   "stale inference image"])
def test_assert_pure_refuses(spoil):
    trace, replayed = _run(spoil)
    with pytest.raises(AssertionError):
        TR.assert_pure(trace, replayed, LAYOUT, _moving())


def test_assert_pure_names_the_step_and_the_tensor():
    trace, replayed = _run("bit flip at step 3")
    with pytest.raises(AssertionError, match=r"step 3 \(train, batch 6\): gradients .* first in b_b, 1 entries in all"):
        TR.assert_pure(trace, replayed, LAYOUT, _moving())


def test_assert_pure_refuses_a_reset_that_keeps_gradients_readable_or_moments():
    trace, replayed = _run(None)
    bad = list(trace)
    bad[9] = bad[9]._replace(out=(None,))
    with pytest.raises(AssertionError, match="AZR_E_STATE"):
        TR.assert_pure(bad, replayed, LAYOUT, _moving())
    trace, replayed = _run("m, v kept through reset")
    with pytest.raises(AssertionError, match=r"step 10 \(train, batch 4\): first step on cleared optimiser state"):
        TR.assert_pure(trace, replayed, LAYOUT, _moving())


@pytest.mark.parametrize("spoil", ["m zeroed by a rebuild", "t restarts at a rebuild", "m, v kept through reset"])
def test_adam_trajectory_refuses(spoil):
    trace, replayed = _run(spoil)
    with pytest.raises(AssertionError, match="Adam"):
        TR.adam_trajectory(trace, KINDS)


def test_first_difference_and_default_layout():
    a = np.zeros(COUNT, f32)
    b = a.copy()
    assert TR.first_difference(a, b, LAYOUT) is None
    b[30] = -0.0                                         # equal as numbers, not as bits
    b[62] = 1
    assert TR.first_difference(a, b, LAYOUT) == ("a_bn", 2)
    lay, n = TR.train.layout(2)
    assert TR._layout_of(n) == lay and (TR.kinds(2) == 0).sum() == 2 * 7 + 4 * 512 + 2 * 2 + 2 * 1
