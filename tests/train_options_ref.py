"""The optimiser step's options restated on the host (TEST INFRASTRUCTURE, not collected): the learning-rate schedule, the clip scale of
tf.clip_by_global_norm, Adam with the rate, the L2 coefficient and the clip scale as parameters (train_replay.tf_adam's arithmetic, which
is the special case lr_t(t, DEFAULTS), l2 = 1e-3, s = 1), and the EMA recurrence.  The formulae are those of include/azr.h; the schedule
is evaluated in float64 as the device evaluates it, Adam and the EMA in float32.  Its own checks: tests/test_train_options.py."""
import numpy as np

import train_replay as TR

f32 = np.float32
LR_CONSTANT, LR_COSINE, LR_STEP = 0, 1, 2
B1, B2, EPS = 0.9, 0.999, 1e-8
B1_F32, B2_F32 = float(f32(B1)), float(f32(B2))   # the step's constants are fp32 values: its bias correction raises THESE to the power t, in double
DEFAULTS = dict(lr=1e-3, l2=1e-3, lr_schedule=LR_CONSTANT, warmup_steps=0, total_steps=0, decay_period=1, decay_gamma=1.0, lr_min=0.0,
                clip_norm=0.0, ema_decay=0.0)
# through the new kernels, and the default step's bits: every factor is exactly 1 (clip_norm is far above any norm, the EMA is a side output)
NEUTRAL = dict(lr=1e-3, l2=1e-3, lr_schedule=LR_CONSTANT, clip_norm=1e30, ema_decay=0.5)


def options(**kw):
    """DEFAULTS with the given fields replaced; float fields as the fp32 values the C struct holds"""
    assert set(kw) <= set(DEFAULTS), set(kw) - set(DEFAULTS)
    o = dict(DEFAULTS, **kw)
    return {k: (float(f32(v)) if isinstance(DEFAULTS[k], float) else int(v)) for k, v in o.items()}


def refusal(o):
    """why azr_nn_train_set_options refuses these options (any field may be missing: its default), None if it takes them"""
    o = dict(DEFAULTS, **o)
    if not all(np.isfinite(o[k]) for k in ("lr", "l2", "decay_gamma", "lr_min", "clip_norm", "ema_decay")):
        return "not finite"
    if not o["lr"] > 0:
        return "lr"
    if o["l2"] < 0:
        return "l2"
    if o["lr_schedule"] not in (LR_CONSTANT, LR_COSINE, LR_STEP):
        return "lr_schedule"
    if o["warmup_steps"] < 0:
        return "warmup_steps"
    if o["lr_schedule"] == LR_COSINE and o["total_steps"] <= o["warmup_steps"]:
        return "total_steps"
    if o["lr_schedule"] == LR_COSINE and not 0 <= o["lr_min"] <= o["lr"]:
        return "lr_min"
    if o["lr_schedule"] == LR_STEP and o["decay_period"] < 1:
        return "decay_period"
    if o["lr_schedule"] == LR_STEP and not 0 < o["decay_gamma"] <= 1:
        return "decay_gamma"
    if o["clip_norm"] < 0:
        return "clip_norm"
    if not 0 <= o["ema_decay"] < 1:
        return "ema_decay"
    return None


# every refusal azr_nn_train_set_options documents, one row each: (the fields that differ from the defaults, the field it is refused for)
REFUSED = [
    (dict(lr=float("nan")), "not finite"), (dict(clip_norm=float("inf")), "not finite"), (dict(ema_decay=float("nan")), "not finite"),
    (dict(lr=0.0), "lr"), (dict(lr=-1e-3), "lr"), (dict(l2=-1e-4), "l2"),
    (dict(lr_schedule=3), "lr_schedule"), (dict(lr_schedule=-1), "lr_schedule"), (dict(warmup_steps=-1), "warmup_steps"),
    (dict(lr_schedule=LR_COSINE, warmup_steps=4, total_steps=4), "total_steps"),
    (dict(lr_schedule=LR_COSINE, total_steps=10, lr_min=-1e-4), "lr_min"), (dict(lr_schedule=LR_COSINE, total_steps=10, lr_min=2e-3), "lr_min"),
    (dict(lr_schedule=LR_STEP, decay_period=0, decay_gamma=0.5), "decay_period"),
    (dict(lr_schedule=LR_STEP, decay_period=2, decay_gamma=0.0), "decay_gamma"), (dict(lr_schedule=LR_STEP, decay_period=2, decay_gamma=1.5), "decay_gamma"),
    (dict(clip_norm=-1.0), "clip_norm"), (dict(ema_decay=1.0), "ema_decay"), (dict(ema_decay=-0.1), "ema_decay"),
]


def lr_eff(t, o):
    """the scheduled rate of Adam step t (1-based), float64"""
    W, N = o["warmup_steps"], o["total_steps"]
    warm = min(1.0, t / W) if W > 0 else 1.0
    f = 1.0
    if o["lr_schedule"] == LR_COSINE:
        p = min(1.0, max(0.0, (t - W) / (N - W)))
        r = o["lr_min"] / o["lr"]
        f = r + (1.0 - r) * 0.5 * (1.0 + np.cos(np.pi * p))
    elif o["lr_schedule"] == LR_STEP:
        f = o["decay_gamma"] ** ((t - 1) // o["decay_period"])
    return o["lr"] * warm * f


def lr_t(t, o, b1=B1_F32, b2=B2_F32):
    """the bias-corrected rate Adam multiplies by at step t, as fp32.  (train_replay.tf_adam corrects with the doubles 0.9 and 0.999:
    a rate 6e-6 away in relative terms, far inside ADAM_BOUND, and far outside the one ulp the stats are held to)"""
    return f32(lr_eff(t, o) * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))


def ghat(w, g, k, l2):
    """the gradient of the whole loss in fp32, as the step forms it: g + 2 l2 w on the kernels (kind 1), g on kind 2, nothing on kind 0"""
    w, g = w.astype(f32), g.astype(f32)
    return np.where(k == 1, g + (f32(2) * f32(l2)) * w, np.where(k == 2, g, f32(0))).astype(f32)


def grad_norm(w, g, k, l2):
    """the global norm of ghat, squares and sum in float64"""
    return float(np.sqrt((ghat(w, g, k, l2).astype(np.float64) ** 2).sum()))


def clip_scale(norm, clip_norm):
    """s = clip / max(norm, clip) as fp32; 1 while clipping is off"""
    return f32(1) if clip_norm == 0 else f32(clip_norm / max(norm, clip_norm))


def adam(w, g, m, v, k, lr_t_, l2, s=f32(1)):
    """train_replay.tf_adam with the bias-corrected rate, the L2 coefficient and the clip scale as parameters"""
    w, m, v = (a.astype(f32).copy() for a in (w, m, v))
    gh = ghat(w, g, k, l2) * f32(s)
    tr = k > 0
    m2 = f32(B1) * m + f32(1 - B1) * gh
    v2 = f32(B2) * v + f32(1 - B2) * gh * gh
    w2 = w - f32(lr_t_) * m2 / (np.sqrt(v2) + f32(EPS))
    return np.where(tr, w2, w), np.where(tr, m2, m), np.where(tr, v2, v)


def ema(e, w_new, k, d):
    """e = d e + (1 - d) w_new on the trained slots, e = w_new on the BN moving statistics (kind 0), in fp32"""
    e, w_new, d = e.astype(f32), w_new.astype(f32), f32(d)
    return np.where(k > 0, d * e + (f32(1) - d) * w_new, w_new).astype(f32)


def assert_default_is_tf_adam(blocks=1, seed=0):
    """adam at the default options is train_replay.tf_adam, bit for bit, on random vectors"""
    k = TR.kinds(blocks)
    rng = np.random.default_rng(seed)
    w, g, m = (rng.normal(0, 0.1, len(k)).astype(f32) for _ in range(3))
    v = rng.uniform(0, 0.01, len(k)).astype(f32)
    for t in (1, 2, 7, 1000):
        a = adam(w, g, m, v, k, lr_t(t, DEFAULTS, B1, B2), 1e-3)   # (tf_adam's rate: the doubles 1e-3, 0.9 and 0.999, not the fp32 values)
        b = TR.tf_adam(w, g, m, v, t, k)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), t
