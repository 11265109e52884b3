"""GPU: the optimiser step's options (azr_nn_train_set_options: learning-rate schedule, global-norm clipping, EMA weights) against
their host-side restatement (tests/train_options_ref.py; its own checks run on the CPU in tests/test_train_options.py).
A step is a pure function of weights and minibatch (tests/test_gpu_train_replay.py), so a twin engine on default options supplies, in
advance, the gradients and norms of the steps an engine under test is about to take from the same weights.
Engines: 8 games, NET_F32, B = 1 and B = 2 blocks.  The norm's reduction runs on a fixed grid of 1024 blocks x 256 threads = 262 144
slots per sweep: B = 1 has 1 227 376 parameters, 4 whole sweeps and a last one of 178 800 slots (698 whole blocks, block 698 with 112
threads, the blocks behind it idle); B = 2 has 2 409 072, 9 whole sweeps and a last one of 49 776 (194 whole blocks, block 194 with 112).
Batches of 16 records (t_conv_q), one of 50 (the fp32-MFMA GEMMs)."""
import functools

import numpy as np
import pytest

import azr_testlib as T
import train_options_ref as R
import train_replay as TR
from dp_group import shuffle_perms
from gpu_common import pkg, records

pytestmark = pytest.mark.gpu

f32 = np.float32
E_INVALID, E_STATE = 1, 7
BS = 16


def _engine(blocks, **opts):
    P = pkg()
    e = P.Engine(8, blocks=blocks, sims=1, dtype=P.NET_F32, node_capacity=64)
    e.set_weights(_flat(blocks))
    if opts:
        e.train_set_options(**opts)
    return e


@functools.lru_cache(maxsize=None)
def _flat(blocks):
    return T.make_net_flat(blocks, seed=11, perturb_bn=True)


@functools.lru_cache(maxsize=None)
def _rec():
    return records(160, seed=41)


def _batch(i, bs=BS):
    return _rec()[i * BS:i * BS + bs]


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _stats_bytes(st):
    return np.array([st[k] for k in sorted(st)], np.float64).tobytes()


@functools.lru_cache(maxsize=None)
def _twin(blocks):
    """three steps of an engine that never heard of options, on batches 0, 1, 2: per step (weights before, raw gradients, weights behind,
    stats behind), and the float64 norm of the whole loss's gradient.  Computed once; callers must not write into it"""
    e = _engine(blocks)
    k = TR.kinds(blocks)
    out = []
    for i in range(3):
        w0 = e.get_weights()
        e.train_batch(_batch(i))
        g = e.train_grads()
        out.append(dict(w0=w0, g=g, w1=e.get_weights(), stats=e.train_stats(), norm=R.grad_norm(w0, g, k, 1e-3)))
    e.close()
    return out


def _ulp_close(a, b, ulps=1):
    return abs(float(f32(a)) - float(f32(b))) <= ulps * float(np.spacing(f32(abs(b))))


@pytest.mark.parametrize("blocks", [1, 2])
def test_defaults_are_the_parents_step(blocks):
    """explicit defaults through the setter: the same bits as an engine that never called it, over three steps; the stats of the default path"""
    tw = _twin(blocks)
    e = _engine(blocks)
    e.train_set_options()
    assert e.train_options() == R.options()
    for i in range(3):
        e.train_batch(_batch(i))
        assert (_bits(e.get_weights()) == _bits(tw[i]["w1"])).all(), i
        st = e.train_stats()
        assert st["step"] == i + 1 and st["lr"] == float(f32(1e-3)) and np.isnan(st["grad_norm"]) and st["clip_scale"] == 1.0
        assert st["clipped_steps"] == 0 and st["ema_steps"] == 0
        assert _ulp_close(st["lr_t"], R.lr_t(i + 1, R.options()))
        assert _stats_bytes(st) == _stats_bytes(tw[i]["stats"])
    e.close()


@pytest.mark.parametrize("blocks", [1, 2])
def test_neutral_options_through_the_new_kernels(blocks):
    """lr, l2 at their defaults, CONSTANT, a clip norm nothing reaches, EMA on: t_grad_sqsum, t_tick_lr_sched and t_adam_opt run, every
    factor is exactly 1, and the weights are the default engine's bit for bit.  grad_norm against the float64 norm of the fp32 gradient
    of the whole loss built from train_grads(): every fp32 term is within 2^-23 and the cast within 2^-24, hence 5e-7 relative"""
    tw = _twin(blocks)
    k = TR.kinds(blocks)
    e = _engine(blocks, **R.NEUTRAL)
    for i in range(3):
        w0 = e.get_weights()
        e.train_batch(_batch(i))
        assert (_bits(e.get_weights()) == _bits(tw[i]["w1"])).all(), (i, int((_bits(e.get_weights()) != _bits(tw[i]["w1"])).sum()))
        st = e.train_stats()
        assert st["clip_scale"] == 1.0 and st["clipped_steps"] == 0 and st["ema_steps"] == i + 1 and st["step"] == i + 1
        assert st["lr"] == float(f32(1e-3)) and f32(st["lr_t"]) == f32(tw[i]["stats"]["lr_t"])
        want = R.grad_norm(w0, e.train_grads(), k, 1e-3)
        print("B = %d step %d: grad_norm %.9g, float64 %.9g, relative %.2e" % (blocks, i + 1, st["grad_norm"], want, abs(st["grad_norm"] - want) / want))
        assert abs(st["grad_norm"] - want) <= 5e-7 * want
        assert abs(want - tw[i]["norm"]) <= 1e-12 * want     # the twin's norm is the norm of this step: same weights, same batch
    e.close()


def _clip_run(blocks, factor):
    """step 1 with clipping off, step 2 with clip_norm = factor * the twin's norm of step 2: (weights behind step 1, behind step 2, raw
    gradients of step 2, stats behind step 2, the clip norm as the fp32 value the engine holds)"""
    clip = float(f32(factor * _twin(blocks)[1]["norm"]))
    e = _engine(blocks)
    e.train_batch(_batch(0))
    w1 = e.get_weights()
    e.train_set_options(clip_norm=clip)
    e.train_batch(_batch(1))
    out = (w1, e.get_weights(), e.train_grads(), e.train_stats(), clip)
    e.close()
    return out


_clipped = functools.lru_cache(maxsize=None)(_clip_run)


@pytest.mark.parametrize("blocks", [1, 2])
def test_clipping_scales_the_gradient_adam_sees(blocks):
    """Adam's first step is nearly invariant to a gradient scale (m / sqrt(v) = g / |g|), so the SECOND step is clipped, to a quarter of
    its norm: the restated Adam on s * g^ lands within ADAM_BOUND, the one without s misses by more than a hundred times that — a
    dropped scale would not pass.  A clip norm of twice the norm then leaves the twin's bits."""
    tw, k = _twin(blocks), TR.kinds(blocks)
    tr = k > 0
    w1, w2, g2, st, clip = _clipped(blocks, 0.25)
    assert (_bits(w1) == _bits(tw[0]["w1"])).all() and (_bits(g2) == _bits(tw[1]["g"])).all()
    assert 0.2 < st["clip_scale"] < 0.3 and st["clipped_steps"] == 1 and st["step"] == 2
    assert abs(st["grad_norm"] - tw[1]["norm"]) <= 5e-7 * tw[1]["norm"]
    s = R.clip_scale(tw[1]["norm"], clip)
    assert _ulp_close(st["clip_scale"], s, 2)
    zero = np.zeros(len(k), f32)
    _, m1, v1 = R.adam(tw[0]["w0"], tw[0]["g"], zero, zero, k, R.lr_t(1, R.options()), 1e-3)
    with_s = R.adam(w1, g2, m1, v1, k, R.lr_t(2, R.options()), 1e-3, s)[0]
    without = R.adam(w1, g2, m1, v1, k, R.lr_t(2, R.options()), 1e-3)[0]
    dev, miss = float(np.abs(w2[tr] - with_s[tr]).max()), float(np.abs(w2[tr] - without[tr]).max())
    print("B = %d: clip_scale %.6f; weights %.2e from Adam on s * g^ (bound %.0e), %.2e from Adam on g^" % (blocks, st["clip_scale"], dev, TR.ADAM_BOUND, miss))
    assert dev <= TR.ADAM_BOUND
    assert miss > 100 * TR.ADAM_BOUND
    assert (_bits(w2)[~tr] == _bits(tw[1]["w1"])[~tr]).all()      # the moving statistics are the forward pass's, clipped or not
    _, w2x, _, stx, _ = _clip_run(blocks, 2.0)
    assert stx["clip_scale"] == 1.0 and stx["clipped_steps"] == 0
    assert (_bits(w2x) == _bits(tw[1]["w1"])).all()


@pytest.mark.parametrize("blocks", [1, 2])
def test_clipped_step_is_reproducible(blocks):
    """the norm's sum has a fixed order and no atomics: the clipped schedule on another fresh engine gives the same bytes"""
    a, b = _clipped(blocks, 0.25), _clip_run(blocks, 0.25)
    assert a[1].tobytes() == b[1].tobytes() and _stats_bytes(a[3]) == _stats_bytes(b[3])


def _follow(e, o, k, steps, bound, first=0):
    """`steps` single steps on batches first, first + 1, ...: stats.lr and stats.lr_t within one fp32 ulp of the restated schedule, the
    weights within `bound` of the restated Adam on the engine's own gradients and weights (m, v carried here); returns the worst deviation"""
    tr = k > 0
    m, v = np.zeros(len(k), f32), np.zeros(len(k), f32)
    worst = 0.0
    for t in range(1, steps + 1):
        w0 = e.get_weights()
        e.train_batch(_batch(first + t - 1))
        st = e.train_stats()
        assert st["step"] == t
        assert _ulp_close(st["lr"], R.lr_eff(t, o)) and _ulp_close(st["lr_t"], R.lr_t(t, o)), (t, st, R.lr_eff(t, o), R.lr_t(t, o))
        w, m, v = R.adam(w0, e.train_grads(), m, v, k, R.lr_t(t, o), o["l2"])
        dev = float(np.abs(e.get_weights()[tr] - w[tr]).max())
        assert dev <= bound, (t, dev)
        worst = max(worst, dev)
    return worst


COSINE = dict(lr_schedule=R.LR_COSINE, warmup_steps=3, total_steps=6, lr_min=1e-4)


def test_cosine_schedule_and_its_restart():
    """warm-up over 3 steps, cosine down to a tenth of the rate at step 6, flat behind it: 7 single steps; azr_nn_train_reset restarts
    the schedule with Adam's step count"""
    o, k = R.options(**COSINE), TR.kinds(1)
    e = _engine(1, **COSINE)
    worst = _follow(e, o, k, 7, TR.ADAM_BOUND)
    assert f32(e.train_stats()["lr"]) == f32(1e-4)
    print("cosine: worst deviation from the restated Adam %.2e" % worst)
    e.train_reset()
    with pytest.raises(pkg().AzrError) as ei:
        e.train_stats()
    assert ei.value.code == E_STATE
    assert e.train_options() == o
    _follow(e, o, k, 2, TR.ADAM_BOUND, first=7)
    e.close()


def test_step_schedule():
    o = R.options(lr_schedule=R.LR_STEP, decay_period=2, decay_gamma=0.5)
    e = _engine(1, lr_schedule=R.LR_STEP, decay_period=2, decay_gamma=0.5)
    _follow(e, o, TR.kinds(1), 5, TR.ADAM_BOUND)
    assert e.train_stats()["lr"] == float(f32(1e-3)) / 4
    e.close()


def test_epoch_loop_evaluates_the_schedule_on_the_device():
    """azr_nn_train queues 2 epochs x 3 steps back to back: the schedule comes from the device's step count, no host round trip.
    Against six train_batch calls driven by std::shuffle's permutations: weights equal as uint32, the same stats"""
    n, state = 3 * BS + 5, 20260007
    rec = _rec()[:n]
    perms, end = shuffle_perms(n, state, 2)
    a, b = _engine(1, **COSINE), _engine(1, **COSINE)
    hist, st = a.train(rec, 2, batch_size=BS, rng_state=state)
    assert st == end
    for ep in range(2):
        for c in range(3):
            b.train_batch(rec[perms[ep][c * BS:(c + 1) * BS]])
    assert (_bits(a.get_weights()) == _bits(b.get_weights())).all()
    assert a.train_stats()["step"] == 6 and _stats_bytes(a.train_stats()) == _stats_bytes(b.train_stats())
    assert f32(a.train_stats()["lr"]) == f32(1e-4)
    a.close(); b.close()


def test_lr_and_l2_are_values():
    """lr = 3e-4, l2 = 0 over two steps: within ADAM_BOUND * max(1, lr / 1e-3) of the restatement; the restatement at the default values
    misses by more than a hundred times that"""
    o, k = R.options(lr=3e-4, l2=0.0), TR.kinds(1)
    tr = k > 0
    bound = TR.ADAM_BOUND * max(1.0, o["lr"] / 1e-3)
    e = _engine(1, lr=3e-4, l2=0.0)
    m = v = md = vd = np.zeros(len(k), f32)
    for t in (1, 2):
        w0 = e.get_weights()
        e.train_batch(_batch(t - 1))
        g, w1 = e.train_grads(), e.get_weights()
        w, m, v = R.adam(w0, g, m, v, k, R.lr_t(t, o), o["l2"])
        wd, md, vd = R.adam(w0, g, md, vd, k, R.lr_t(t, R.options()), 1e-3)
        dev, miss = float(np.abs(w1[tr] - w[tr]).max()), float(np.abs(w1[tr] - wd[tr]).max())
        print("step %d: %.2e from Adam(3e-4, l2 0) (bound %.1e), %.2e from Adam at the defaults" % (t, dev, bound, miss))
        assert dev <= bound and miss > 100 * bound
    assert e.train_stats()["lr"] == o["lr"]
    e.close()


def test_ema_follows_the_recurrence_through_context_rebuilds():
    """d = 0.75 over train 16, train 16, validate 48, train 50, train 16: the vector is optimiser state and lives through the rebuilds of
    the training context.  After every step e is within 2^-22 * max(|e_prev|, |w_new|) of d * e_prev + (1 - d) * w_new, e_prev the
    device's own previous vector (three fp32 roundings per step, no drift adds up); the moving statistics are the weights' bit for bit"""
    P, k, d = pkg(), TR.kinds(2), 0.75
    e = _engine(2, ema_decay=d)
    with pytest.raises(P.AzrError) as ei:
        e.get_ema_weights()
    assert ei.value.code == E_STATE
    prev, at, steps = e.get_weights(), 0, 0     # the vector starts as the weights from before its first step
    for kind, bs in (("train", 16), ("train", 16), ("validate", 48), ("train", 50), ("train", 16)):
        r = _rec()[at:at + bs]
        at += bs
        if kind == "validate":
            before = e.train_stats()
            e.validate(r, batch_size=bs)
            assert e.get_ema_weights().tobytes() == prev.tobytes()
            assert _stats_bytes(e.train_stats()) == _stats_bytes(before)     # the stats are the last STEP's, whatever was rebuilt since
            continue
        e.train_batch(r)
        steps += 1
        w, got = e.get_weights(), e.get_ema_weights()
        want = R.ema(prev, w, k, d)
        assert (np.abs(got - want) <= 2.0 ** -22 * np.maximum(np.abs(prev), np.abs(w))).all(), (steps, float(np.abs(got - want).max()))
        assert (_bits(got)[k == 0] == _bits(w)[k == 0]).all()
        assert np.abs(got - w)[k > 0].max() > 1e-5          # an average, not a copy of the weights
        assert e.train_stats()["ema_steps"] == steps and e.train_stats()["step"] == steps
        prev = got
    other = P.Engine(8, blocks=2, sims=1, dtype=P.NET_F32, node_capacity=64)
    other.set_weights(prev)                                  # an AZRW vector like any other
    pi, v = other.predict(_rec()[:8, 1:89].copy())
    assert np.isfinite(pi).all() and np.isfinite(v).all() and np.allclose(pi.sum(1), 1, atol=1e-5)
    other.close()
    e.train_reset()
    with pytest.raises(P.AzrError) as ei:
        e.get_ema_weights()
    assert ei.value.code == E_STATE
    e.close()


def test_refused_options_leave_the_previous_ones():
    P = pkg()
    e = _engine(1)
    good = dict(lr=2e-3, clip_norm=1.0, lr_schedule=R.LR_STEP, decay_period=3, decay_gamma=0.5)
    e.train_set_options(**good)
    for o, why in R.REFUSED:
        with pytest.raises(P.AzrError) as ei:
            e.train_set_options(**o)
        assert ei.value.code == E_INVALID and "azr_nn_train_set_options" in str(ei.value), (o, why)
        assert e.train_options() == R.options(**good), (o, why)
    e.train_set_options(lr_schedule="cosine", total_steps=10)   # by name
    assert e.train_options()["lr_schedule"] == R.LR_COSINE
    e.close()
