"""CPU: the host-side restatement of the optimiser step's options (tests/train_options_ref.py) checked on its own, the binding's view
of azr_train_options / azr_train_stats, and learn.py's flags: parsed into the options, and refused before an engine exists where
azr_nn_train_set_options would refuse them."""
import argparse
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import train_options_ref as R
from gpu_common import pkg, ROOT
from host_cli import check_learn_py_lists, check_learn_py_rejects

f32 = np.float32


def test_warmup_reaches_the_rate_exactly_at_w():
    o = R.options(lr=3e-4, warmup_steps=5)
    assert [R.lr_eff(t, o) / o["lr"] for t in (1, 2, 5)] == [1 / 5, 2 / 5, 1.0]
    assert all(R.lr_eff(t, o) == o["lr"] for t in (5, 6, 1000))
    assert all(R.lr_eff(t, R.options(lr=3e-4)) == o["lr"] for t in (1, 2, 1000))   # W = 0: no warm-up


def test_cosine_runs_from_lr_at_w_to_lr_min_from_n_on():
    o = R.options(lr_schedule=R.LR_COSINE, warmup_steps=3, total_steps=6, lr_min=1e-4)
    assert R.lr_eff(3, o) == o["lr"]
    assert [R.lr_eff(t, o) / o["lr"] for t in (1, 2)] == [1 / 3, 2 / 3]   # under the warm-up the cosine is still at 1
    mid = [R.lr_eff(t, o) for t in (3, 4, 5, 6)]
    assert all(a > b for a, b in zip(mid, mid[1:]))
    assert abs(R.lr_eff(4, o) - (o["lr_min"] + (o["lr"] - o["lr_min"]) * 0.75)) < 1e-18   # cos(pi / 3) = 1 / 2
    # lr * (lr_min / lr) is lr_min to the last bit or the one before: one value for every t >= N, and lr_min as fp32
    assert len({R.lr_eff(t, o) for t in (6, 7, 100, 10 ** 6)}) == 1
    assert abs(R.lr_eff(6, o) - o["lr_min"]) <= np.spacing(o["lr_min"]) and f32(R.lr_eff(6, o)) == f32(o["lr_min"])
    assert R.lr_eff(9, R.options(lr_schedule=R.LR_COSINE, total_steps=4)) == 0.0   # lr_min = 0: cos(pi) is -1 exactly


def test_step_schedule_is_a_staircase():
    o = R.options(lr_schedule=R.LR_STEP, decay_period=2, decay_gamma=0.5)
    assert [R.lr_eff(t, o) / o["lr"] for t in range(1, 8)] == [1, 1, 0.5, 0.5, 0.25, 0.25, 0.125]
    o = R.options(lr_schedule=R.LR_STEP, decay_period=3, decay_gamma=0.5, warmup_steps=2)
    assert [R.lr_eff(t, o) / o["lr"] for t in range(1, 6)] == [0.5, 1, 1, 0.5, 0.5]


def test_bias_corrected_rate_is_tf_adams():
    for t in (1, 2, 10, 5000):
        assert R.lr_t(t, R.DEFAULTS, R.B1, R.B2) == f32(1e-3 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t))
        assert abs(float(R.lr_t(t, R.options())) / float(R.lr_t(t, R.DEFAULTS, R.B1, R.B2)) - 1) < 1e-5   # the fp32 constants' rate: 6e-6 away at t = 1
    R.assert_default_is_tf_adam()


def test_clip_scale():
    assert R.clip_scale(3.0, 0.0) == 1 and R.clip_scale(3.0, 5.0) == 1 and R.clip_scale(5.0, 5.0) == 1
    assert R.clip_scale(float(f32(0.3)), float(f32(0.3))) == 1
    assert R.clip_scale(20.0, 5.0) == f32(0.25)
    k = np.array([1, 2, 0, 1], np.uint8)
    w, g = np.array([1, 1, 7, -2], f32), np.array([3, 4, 9, 0.5], f32)
    gh = R.ghat(w, g, k, 0.25)      # kind 0 takes no part; kernels carry 2 * l2 * w
    assert gh.tolist() == [3.5, 4, 0, -0.5] and R.grad_norm(w, g, k, 0.25) == np.sqrt(3.5 ** 2 + 16 + 0.25)
    # Adam on s * ghat: a scale moves the moments, not only the step
    a = R.adam(w, g, np.zeros(4, f32), np.zeros(4, f32), k, f32(1e-3), 0.25, s=f32(0.5))
    assert a[1].tolist() == (f32(0.1) * (gh * f32(0.5))).tolist() and a[0][2] == 7 and a[1][2] == 0


def test_ema_recurrence():
    k = np.array([1, 2, 0], np.uint8)
    e = R.ema(np.array([1, 2, 3], f32), np.array([5, 6, 7], f32), k, 0.75)
    assert e.tolist() == [2, 3, 7] and e.dtype == f32


def test_refusals_of_the_restatement_name_the_field():
    assert R.refusal({}) is None and R.refusal(R.NEUTRAL) is None
    assert R.refusal(dict(lr_schedule=R.LR_COSINE, warmup_steps=3, total_steps=6, lr_min=1e-4)) is None
    assert R.refusal(dict(total_steps=0, lr_min=5.0, decay_period=0, decay_gamma=7.0)) is None   # not read under CONSTANT
    for o, why in R.REFUSED:
        assert R.refusal(o) == why, (o, why)


def test_binding_structs_mirror_the_header():
    """field for field: names, order and C types of azr_train_options and azr_train_stats, the schedule enumerators, the defaults"""
    P = pkg()
    hdr = open(os.path.join(ROOT, "include", "azr.h")).read()
    ctype = {"float": C.c_float, "int32_t": C.c_int32, "int64_t": C.c_int64}
    for name, cls in (("azr_train_options", P.TrainOptions), ("azr_train_stats", P.TrainStats)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [(n.strip(), ctype[t]) for t, names in re.findall(r"(\w+)\s+([\w,\s]+);", body) for n in names.split(",")]
        assert fields == list(cls._fields_), name
    vals = {k: int(v) for k, v in re.findall(r"\b(AZR_LR_[A-Z]+)\s*=\s*(\d+)", hdr)}
    assert vals == {"AZR_LR_CONSTANT": P.LR_CONSTANT, "AZR_LR_COSINE": P.LR_COSINE, "AZR_LR_STEP": P.LR_STEP}
    assert P.LR_SCHEDULES == {"constant": R.LR_CONSTANT, "cosine": R.LR_COSINE, "step": R.LR_STEP}
    o = P.TrainOptions()
    P.load_library().azr_default_train_options(C.byref(o))
    assert o.as_dict() == R.options()


# ---- learn.py ------------------------------------------------------------------------------------------------------------------------
FLAGS = ["--lr", "--l2", "--lr-schedule", "--lr-warmup", "--lr-steps", "--lr-min", "--lr-period", "--lr-gamma", "--clip-norm", "--ema-decay", "--ema-play"]


def _learn():
    return importlib.import_module("alphazero-risk_amd.learn")


def test_learn_py_flag_table():
    """a table of its own: no row of the self-play table, every field of azr_train_options once, the defaults are the C defaults"""
    L = _learn()
    names = [f.name for _, f in L.TRAIN_OPTIONS] + [L.EMA_PLAY.name]
    assert names == FLAGS and not set(n[2:].replace("-", "_") for n in names) & set(L.SELFPLAY_FLAGS)
    assert sorted(field for field, _ in L.TRAIN_OPTIONS) == sorted(n for n, _ in pkg().TrainOptions._fields_)
    ap = argparse.ArgumentParser()
    L.add_train_flags(ap)
    kw, play = L.train_options_of(ap.parse_args([]))
    assert play == 0 and L.train_options_error(kw, play) is None
    assert {k: (pkg().LR_SCHEDULES[v] if k == "lr_schedule" else v) for k, v in kw.items()} == R.DEFAULTS
    kw, play = L.train_options_of(ap.parse_args("--lr 3e-4 --l2 0 --lr-schedule cosine --lr-warmup 3 --lr-steps 6 --lr-min 3e-5 --lr-period 4 --lr-gamma 0.5 "
                                                "--clip-norm 1 --ema-decay 0.999 --ema-play 1".split()))
    assert kw == dict(lr=3e-4, l2=0.0, lr_schedule="cosine", warmup_steps=3, total_steps=6, lr_min=3e-5, decay_period=4, decay_gamma=0.5, clip_norm=1.0,
                      ema_decay=0.999) and play == 1 and L.train_options_error(kw, play) is None
    assert L.train_options_of(argparse.Namespace()) == ({field: f.default for field, f in L.TRAIN_OPTIONS}, 0)   # a caller's bare namespace


def test_learn_py_refuses_what_set_options_refuses():
    """every row of the restatement's refusal list, through learn.py's own check (no process, no engine)"""
    L = _learn()
    sched = {v: k for k, v in pkg().LR_SCHEDULES.items()}
    for o, why in R.REFUSED:
        if why == "lr_schedule":
            continue            # an unknown schedule name never gets past argparse's choices (test below)
        kw = dict(L.train_options_of(argparse.Namespace())[0], **o)
        kw["lr_schedule"] = sched.get(kw["lr_schedule"], kw["lr_schedule"])
        msg = L.train_options_error(kw)
        flag = dict((field, f.name) for field, f in L.TRAIN_OPTIONS)[next(iter(o)) if why == "not finite" else why]
        assert msg is not None and msg.startswith(flag + ":"), (o, why, msg)
    kw = L.train_options_of(argparse.Namespace())[0]
    assert L.train_options_error(kw, 1).startswith("--ema-play:") and L.train_options_error(dict(kw, ema_decay=0.9), 1) is None
    assert L.train_options_error(dict(kw, ema_decay=0.9), 2).startswith("--ema-play:")


@pytest.mark.parametrize("args,flag,why", [
    (["--lr", "0"], "--lr", "learning rate"),
    (["--lr-schedule", "cosine", "--lr-warmup", "5", "--lr-steps", "5"], "--lr-steps", "above --lr-warmup"),
    (["--lr-schedule", "linear"], "--lr-schedule", "invalid choice"),
    (["--clip-norm", "nan"], "--clip-norm", "finite"),
    (["--ema-play", "1"], "--ema-play", "--ema-decay"),
])
def test_learn_py_command_line_rejects(tmp_path, args, flag, why):
    check_learn_py_rejects(tmp_path, args, flag, why)


def test_learn_py_help_lists_the_flags():
    check_learn_py_lists(FLAGS, "tf.clip_by_global_norm")


def test_optimiser_line():
    L = _learn()
    st = dict(step=30, lr=0.00025, lr_t=0.0003, grad_norm=1.5, clip_scale=0.5, clipped_steps=7, ema_steps=30)
    assert L.optimiser_line(st, 10) == "Optimiser step: lr 0.00025, grad norm 1.5, clipped 7/30 steps   [10 steps in this phase]"
    assert "grad norm n/a" in L.optimiser_line(dict(st, grad_norm=float("nan")), 10)
