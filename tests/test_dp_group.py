"""CPU: the checks of tests/dp_group.py on made-up ranks (numpy only), so that the proof the data-parallel optimiser-step tests rest on
cannot pass when it should not: an honest group is accepted, and every seeded defect is refused by the check written for it — by
its message.  The fake rank has what azr_nn_train_dp has: a shuffle in front of the steps (the same libstdc++ probe), a slice of every
minibatch by rank, three sums per step through the callback (float64 statistics, the float32 loss pair, the gradient vector), a
training context per share that carries Adam's state, and a plain single-rank step."""
import threading
import time

import numpy as np
import pytest

import dp_group as DG
import train_replay as TR

f32 = np.float32
LAYOUT = [("a_w", 0, (3, 8)), ("a_bn", 24, (4, 5)), ("b_w", 44, (16,)), ("b_b", 60, (4,))]
COUNT = 64
KINDS = np.zeros(COUNT, np.uint8)
KINDS[0:24] = 1; KINDS[24:34] = 2; KINDS[44:60] = 1; KINDS[60:64] = 2
NSTAT = 8
PER_STEP = 3
SCHEDULE = [("train", 8), ("train", 8), ("validate", 6, 2), ("train", 8), ("train", 20), ("solo", 8), ("train", 20), ("predict", 3),
            ("train", 4), ("reset",), ("train", 4), ("train", 8)]
SCHEDULE3 = [("train", 12), ("train", 12), ("train", 6), ("validate", 6, 1), ("solo", 5), ("train", 6), ("reset",), ("train", 12), ("train", 6)]


class FakeError(RuntimeError):
    def __init__(self, code):
        super().__init__("fake error %d" % code)
        self.code = code


def _terms(w, my, feat):
    """per-record loss terms of the records `my` under the whole batch's statistic `feat`"""
    f = my[:, :COUNT].astype(f32) / f32(255)
    return (f * np.tanh(w)).mean(1).astype(f32), ((f - feat) ** 2).mean(1).astype(f32)


def reference_terms(w, rec):
    """the same terms in float64 for a whole minibatch: what assert_membership compares the ranks' contributions with"""
    w, r = np.asarray(w, np.float64), np.asarray(rec, np.float64)
    feat = np.resize(((r[:, :NSTAT] / 255).sum(0) / len(r)).astype(f32), COUNT).astype(np.float64)
    f = r[:, :COUNT] / 255
    return (f * np.tanh(w)).mean(1), ((f - feat) ** 2).mean(1)


class FakeRank:
    """one rank; spoil names the one defect it has"""

    def __init__(self, spoil=None):
        self.spoil = spoil
        self.share = None              # the training context: the share it was built for, Adam state, last gradients
        self.m = self.v = self.g = None
        self.t = 0
        self.world, self.rank = 1, 0   # what the running call set
        self.seen_rank = 0             # the rank of the last data-parallel call
        self.dp_steps = 0

    def set_weights(self, w):
        self.w = np.array(w, f32)

    def get_weights(self):
        w = self.w.copy()
        if self.spoil == "one bit of rank 1's weights" and self.seen_rank == 1 and self.dp_steps >= 2:
            w[17:18].view(np.uint32)[0] ^= 1
        return w

    def _ensure(self, share):
        if self.share == share:
            return
        if self.share is None:
            self.m, self.v, self.t = np.zeros(COUNT, f32), np.zeros(COUNT, f32), 0
        elif self.spoil == "moments zeroed when the share changes":
            self.m, self.v = np.zeros(COUNT, f32), np.zeros(COUNT, f32)
        self.share, self.g = share, np.zeros(COUNT, f32)

    def _step(self, my, bs, ar, skip_last=False):
        s = (my[:, :NSTAT].astype(np.float64) / 255).sum(0)
        if ar:
            ar(s, NSTAT, 1)
        feat = np.resize((s / bs).astype(f32), COUNT)
        tp, tv = _terms(self.w, my, feat)
        loss = np.array([tp.sum(dtype=f32) / f32(bs), tv.sum(dtype=f32) / f32(bs)], f32)
        if ar:
            ar(loss, 2, 0)
        f = my[:, :COUNT].astype(f32) / f32(255)
        g = ((np.tanh(self.w) * f32(0.25) - f32(0.4)) * f32(len(my)) + (f * (f32(1) + feat)).sum(0, dtype=f32)) / f32(bs)
        g = np.where(KINDS > 0, g, f32(0)).astype(f32)
        if ar and not skip_last:
            ar(g, COUNT, 0)
        self.t += 1
        w, self.m, self.v = TR.tf_adam(self.w, g, self.m, self.v, self.t, KINDS)
        mov = KINDS == 0
        w[mov] = (f32(0.99) * self.w + f32(0.01) * feat)[mov]
        self.w, self.g = w.astype(f32), g
        return loss

    def train_dp(self, rec, epochs, allreduce, rank, world, batch_size=512, rng_state=None):
        n, share = len(rec), batch_size // world
        assert batch_size % world == 0 and share >= 2
        perms, end = DG.shuffle_perms(n, rng_state, epochs)
        self._ensure(share)
        self.world, self.rank, self.seen_rank = world, rank, rank
        take = {"slice shifted by one rank": (rank + 1) % world, "rank 1 takes rank 0's slice": 0 if rank == 1 else rank}.get(self.spoil, rank)
        hist, nb = [], n // batch_size
        for e in range(epochs):
            off, acc = 0, np.zeros(2, f32)
            for _ in range(nb):
                self.dp_steps += 1
                idx = perms[e][off + take * share:off + (take + 1) * share]
                acc += self._step(rec[idx], batch_size, allreduce,
                                  skip_last=self.spoil == "one all-reduce fewer on rank 1" and rank == 1 and self.dp_steps == 2)
                off += share if self.spoil == "offset advanced by the share" else batch_size
            hist.append((float(acc[0] / f32(nb)), float(acc[1] / f32(nb))) if nb else (float("nan"), float("nan")))
        if self.spoil != "world and rank kept in a solo step":
            self.world, self.rank = 1, 0
        return hist, end

    def train_batch(self, rec):
        n = len(rec)
        share = n // self.world
        self._ensure(n)
        loss = self._step(rec[self.rank * share:(self.rank + 1) * share], n, None)
        return float(loss[0]), float(loss[1])

    def train_grads(self):
        if self.share is None:
            raise FakeError(TR.E_STATE)
        return self.g.copy()

    def train_reset(self):
        self.share = None

    def validate(self, rec, batch_size, per_record):
        assert per_record and len(rec) % batch_size == 0
        self._ensure(batch_size)
        r = np.asarray(rec, f32) @ np.resize(self.w, rec.shape[1])
        return float(f32(r.mean())), float(f32((r * r).mean())), r.astype(f32), (r * r).astype(f32)

    def predict(self, x):
        p = (np.asarray(x, f32) @ np.resize(self.w, (x.shape[1], 5))).astype(f32)
        return p, p.sum(1).astype(f32)


def _rank_threads():
    return [t for t in threading.enumerate() if t.name.startswith("dp-rank")]


def _maker(world, spoil=None):
    return lambda: DG.DpGroup(world, lambda: FakeRank(spoil), buffers=DG.HostBuffers(), timeout=20.0)


def _inputs(n=200):
    rng = np.random.default_rng(3)
    return rng.normal(0, 0.5, COUNT).astype(f32), rng.integers(0, 256, (n, 265)).astype(np.uint8)


def _check_schedule(world, spoil, schedule=SCHEDULE):
    flat, rec = _inputs()
    make = _maker(world, spoil)
    trace = TR.run_schedule(make, flat, schedule, rec)
    TR.assert_pure(trace, TR.replay(make, trace), LAYOUT, KINDS == 0)
    return trace, TR.adam_trajectory(trace, KINDS)


def _check_epochs(world, spoil, bs=8):
    flat, rec = _inputs(3 * bs + 5)
    DG.epoch_loop_against_single_steps(_maker(world, spoil), flat, rec, bs, 2, 20260003)


def _check_membership(world, spoil, bs=12):
    flat, rec = _inputs(bs)
    g = _maker(world, spoil)()
    g.set_weights(flat)
    g.train_batch(rec)
    DG.assert_calls(g, 1, PER_STEP, COUNT)
    tp, tv = reference_terms(flat, rec)
    return DG.assert_membership(g.loss_parts(), tp, tv)


@pytest.mark.parametrize("world,schedule", [(2, SCHEDULE), (3, SCHEDULE3)])
def test_the_honest_group_passes(world, schedule):
    trace, worst = _check_schedule(world, None, schedule)
    assert [s.kind for s in trace] == [s[0] for s in schedule] and worst <= TR.ADAM_BOUND
    # a solo step is a train step: it ages the engine and moves the weights
    fresh = [s.fresh for s in trace if s.kind in TR.TRAIN_KINDS]
    assert fresh[0] and not any(fresh[1:-2]) and fresh[-2] and not fresh[-1]
    assert all(np.abs(s.w1 - s.w0)[KINDS > 0].max() > 1e-4 for s in trace if s.kind in TR.TRAIN_KINDS)
    _check_epochs(world, None, 4 * world)
    assert _check_membership(world, None) <= 1e-5


DEFECTS = {
    "offset advanced by the share": (_check_epochs, r"epoch 0: losses of the epoch loop"),
    "world and rank kept in a solo step": (_check_schedule, r"solo step: rank 1 differs from rank 0"),
    "moments zeroed when the share changes": (_check_schedule, r"Adam step \d+: weights .* away from Adam on the carried moments"),
    "one bit of rank 1's weights": (_check_schedule, r"get_weights: rank 1 differs from rank 0 \(differing bytes per output: \[1\]\)"),
    "one all-reduce fewer on rank 1": (_check_schedule, r"rank 0: all-reduce 3 (was not joined by every rank: rank 1 returned after 2 all-reduces|cannot complete, rank 1 returned after 2)"),
    "slice shifted by one rank": (_check_membership, r"rank 0 did not take records 0 \.\. 5"),
    "rank 1 takes rank 0's slice": (_check_membership, r"rank [01] did not take records"),
}


@pytest.mark.parametrize("spoil", sorted(DEFECTS))
def test_each_seeded_defect_is_refused_by_its_check(spoil):
    check, message = DEFECTS[spoil]
    t0 = time.monotonic()
    with pytest.raises(AssertionError, match=message):
        check(2, spoil)
    assert time.monotonic() - t0 < 10.0       # refused at once, not by a timeout running out
    assert not _rank_threads()                # every rank thread has ended


def test_a_callback_that_raises_on_one_rank_surfaces_and_ends_the_group():
    flat, rec = _inputs(16)
    g = _maker(2)()
    g.set_weights(flat)
    g.train_batch(rec[:8])
    make = g.ar.make

    def broken(rank):
        ar = make(rank)

        def cb(ptr, count, dtype):
            if rank == 1 and count == 2:
                raise RuntimeError("the transport broke on rank 1")
            ar(ptr, count, dtype)
        return cb

    g.ar.make = broken
    t0 = time.monotonic()
    with pytest.raises(RuntimeError, match="the transport broke on rank 1"):      # the first error, not rank 0's broken barrier
        g.train_batch(rec[8:])
    assert time.monotonic() - t0 < 10.0
    assert g.threads and not any(t.is_alive() for t in g.threads) and not _rank_threads()
    with pytest.raises(DG.DpError, match="get_weights on a group that has failed"):  # no further call
        g.get_weights()


def test_ranks_that_meet_with_different_buffers_are_refused():
    g = DG.DpGroup(2, lambda: FakeRank(), buffers=DG.HostBuffers(), timeout=20.0)
    out = g._each("probe", lambda r, e: None)        # nothing to reduce: every rank returns, nobody waits
    assert out == [None, None]
    with pytest.raises(DG.DpError, match="different buffers"):
        g._each("probe", lambda r, e: g.ar.make(r)(np.zeros(2 + r, f32), 2 + r, 0))
    assert not any(t.is_alive() for t in g.threads)


def test_the_sum_is_taken_in_rank_order_and_the_loss_parts_are_kept():
    g = DG.DpGroup(3, lambda: FakeRank(), buffers=DG.HostBuffers())
    vals = [f32(1e8), f32(1), f32(-1e8)]             # (1e8 + 1) - 1e8 = 0 in float32; any other order gives 1
    bufs = [np.array([v, v], f32) for v in vals]
    g._each("sum", lambda r, e: g.ar.make(r)(bufs[r], 2, 0))
    assert all((b == 0).all() for b in bufs)
    assert [p[0] for p in g.loss_parts()] == vals and g.ar.calls == [[(2, 0)]] * 3


def test_shuffle_perms_and_the_inverse_feed():
    (p1,), end1 = DG.shuffle_perms(10, DG.STATE)
    (q1, q2), end2 = DG.shuffle_perms(10, DG.STATE, 2)
    assert (p1 == q1).all() and sorted(q2) == list(range(10)) and (q1 != q2).any() and end1 != end2
    rec = np.arange(10 * 265, dtype=np.uint32).astype(np.uint8).reshape(10, 265)
    fed = np.empty_like(rec)
    fed[p1] = rec
    assert (fed[p1] == rec).all()
