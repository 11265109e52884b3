"""GPU: azr_nn_validate (csrc/azr_train.hip) — the validation phase of AlphaZeroNN::trainCrossValidation
(alphazero_nn.cpp:512-548): the step's forward and losses with batch norm on the MOVING statistics (TF_INPUT_TRAINING = FALSE),
no update.  Checked against the same graph in PyTorch float64 in eval() mode (tests/torch_train_ref.py::AzrNet), against the
handle's own inference path, and for the absence of side effects."""
import numpy as np
import pytest
import torch

import azr_testlib as T
from gpu_common import pkg, records
import torch_train_ref as train

pytestmark = pytest.mark.gpu
AZR_E_INVALID_ARGUMENT, AZR_E_STATE = 1, 7   # include/azr.h


def eval_flat(blocks, rec, seed):
    """an AZRW vector whose moving statistics are those of a real batch, perturbed: eval BN then keeps activations at the scale of
    training (the fp16-pair forward conv needs that), and differs from the identity and from the batch statistics"""
    flat = T.make_net_flat(blocks, seed=seed, perturb_bn=True)
    net = train.AzrNet(blocks, flat).double()
    net.train()
    in88, _, _ = train.unpack_records(rec[:64])
    keep = train.BN_MOMENTUM_TORCH
    train.BN_MOMENTUM_TORCH = 1.0   # running statistics := this batch's
    try:
        with torch.no_grad():
            net(torch.from_numpy(train.planes_from_in88(in88)).double())
    finally:
        train.BN_MOMENTUM_TORCH = keep
    f = net.to_flat()
    rng = np.random.default_rng(seed + 7)
    for off, c in T.bn_offsets(blocks):
        var = f[off + 3 * c:off + 4 * c].astype(np.float64)
        f[off + 2 * c:off + 3 * c] += (rng.uniform(-0.3, 0.3, c) * np.sqrt(var)).astype(np.float32)
        f[off + 3 * c:off + 4 * c] = (var * rng.uniform(0.6, 1.6, c)).astype(np.float32)
    return f


def torch_eval(blocks, flat, rec, margin=None):
    """per-record cross-entropy and squared error of the float64 graph in eval() mode; margin: smallest non-zero |ReLU input|"""
    net = train.AzrNet(blocks, flat).double()
    net.eval()
    in88, pi, z = train.unpack_records(rec)
    relu0 = train.F.relu

    def relu(t, *a, **k):
        if margin is not None:
            v = t.detach().abs()
            v = v[v > 0]
            if v.numel():
                margin.append(float(v.min()))
        return relu0(t, *a, **k)

    train.F.relu = relu
    try:
        with torch.no_grad():
            logits, v = net(torch.from_numpy(train.planes_from_in88(in88)).double())
    finally:
        train.F.relu = relu0
    ce = -(torch.from_numpy(pi).double() * torch.log_softmax(logits, 1)).sum(1)
    se = (torch.from_numpy(z).double() - v) ** 2
    return ce.numpy(), se.numpy()


def batch_average(terms, bs):
    """the float sum of the batch means (each a float sum in board order / bs) divided by the batch count"""
    nb = len(terms) // bs
    acc = np.float32(0)
    for k in range(nb):
        s = np.float32(0)
        for x in terms[k * bs:(k + 1) * bs]:
            s = np.float32(s + x)
        acc = np.float32(acc + np.float32(s / np.float32(bs)))
    return np.float32(acc / np.float32(nb))


# (blocks, batch size, batches): t_conv_q (<= 128 records), the fp32-gemm path (42 * 10 rows: no multiple of the 32-deep k-tile),
# t_conv_rs, and the full net for one batch.  Bound: 2e-5 * max(1, |ref|), the one the step's losses meet (tests/test_gpu_train.py).
# Measured worst errors (cross-entropy / squared error): (1, 16) 2.0e-7 / 7.8e-7, (2, 64) 2.4e-7 / 1.1e-6, (2, 10) 4.3e-7 / 2.1e-6,
# (2, 256) 4.8e-7 / 2.5e-6, (20, 512) 1.3e-6 / 1.3e-5.
@pytest.mark.parametrize("blocks,bs,nb", [(1, 16, 3), (2, 64, 2), (2, 10, 3), (2, 256, 2), (20, 512, 1)])
def test_validate_matches_torch_eval(blocks, bs, nb):
    P = pkg()
    n = nb * bs + 3   # + a remainder that is dropped
    # the first record seed whose float64 forward keeps every ReLU input 1e-6 away from zero (up to 64 evaluated records, as the step's test; with
    # more the smallest of 1e7 .. 2e8 inputs is below that for every seed — and the forward is continuous in a flipped input: a mask
    # that fp32 rounding flips moves the loss by no more than that input)
    want = 1e-6 if nb * bs <= 64 else 0.0
    for seed in range(blocks + 1, blocks + 33):
        rec = records(n, seed=seed)
        flat = eval_flat(blocks, rec, seed)
        margin = []
        ce, se = torch_eval(blocks, flat, rec[:nb * bs], margin)
        if min(margin) >= want:
            break
    else:
        pytest.fail("no record seed with a ReLU margin of 1e-6")
    eng = P.Engine(8, blocks=blocks, sims=1, node_capacity=64)
    eng.set_weights(flat)
    lp, lv, rp, rv = eng.validate(rec, batch_size=bs, per_record=True)
    assert rp.shape == (nb * bs,) and rv.shape == (nb * bs,)
    err_p = np.abs(rp - ce) / np.maximum(1.0, np.abs(ce))
    err_v = np.abs(rv - se) / np.maximum(1.0, np.abs(se))
    print(f"validate blocks={blocks} bs={bs}: max error ce {err_p.max():.2e} se {err_v.max():.2e}")
    assert err_p.max() <= 2e-5 and err_v.max() <= 2e-5, (err_p.max(), err_v.max())
    # the averages are the reference's float arithmetic over exactly these per-record terms, bit for bit
    assert np.float32(lp).tobytes() == batch_average(rp, bs).tobytes()
    assert np.float32(lv).tobytes() == batch_average(rv, bs).tobytes()
    eng.close()


def test_validate_agrees_with_inference():
    """the eval BN uses the moving statistics the fp32 inference refold uses: predict's pi / v give the same per-record terms"""
    P = pkg()
    blocks, bs = 2, 32
    rec = records(2 * bs, seed=31)
    flat = eval_flat(blocks, rec, 31)
    eng = P.Engine(8, blocks=blocks, sims=1, dtype=P.NET_F32, node_capacity=64)
    eng.set_weights(flat)
    _, _, rp, rv = eng.validate(rec, batch_size=bs, per_record=True)
    in88, pi_t, z = train.unpack_records(rec)
    pi, v = eng.predict(in88)
    ce = -(pi_t.astype(np.float64) * np.log(pi.astype(np.float64))).sum(1)
    se = (z.astype(np.float64) - v.astype(np.float64)) ** 2
    np.testing.assert_allclose(rp, ce, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(rv, se, rtol=1e-4, atol=1e-6)
    eng.close()


def test_validate_has_no_side_effects():
    P = pkg()
    blocks, bs = 1, 32
    rec = records(3 * bs, seed=41)
    val = records(2 * bs + 5, seed=42)
    flat = eval_flat(blocks, rec, 41)
    a = P.Engine(8, blocks=blocks, sims=1, node_capacity=64)
    b = P.Engine(8, blocks=blocks, sims=1, node_capacity=64)
    a.set_weights(flat)
    b.set_weights(flat)
    ha, sa = a.train(rec, 1, batch_size=bs, rng_state=20260001)
    hb, sb = b.train(rec, 1, batch_size=bs, rng_state=20260001)
    x = val[:, 1:89].copy()
    before = a.predict(x)
    r1 = a.validate(val, batch_size=bs, per_record=True)
    r2 = a.validate(val, batch_size=bs, per_record=True)
    after = a.predict(x)
    # validate twice: the same bits
    assert r1[:2] == r2[:2] and r1[2].tobytes() == r2[2].tobytes() and r1[3].tobytes() == r2[3].tobytes()
    # the inference images are untouched
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    # train(1); validate; train(1) == train(1); train(1): weights, moving statistics, Adam moments and step count, shuffle stream
    ha2, sa2 = a.train(rec, 1, batch_size=bs, rng_state=sa)
    hb2, sb2 = b.train(rec, 1, batch_size=bs, rng_state=sb)
    assert (ha, ha2, sa2) == (hb, hb2, sb2)
    assert a.get_weights().tobytes() == b.get_weights().tobytes()
    a.close(); b.close()


def test_validate_edges():
    P = pkg()
    blocks, bs = 1, 16
    rec = records(2 * bs + 5, seed=51)
    eng = P.Engine(8, blocks=blocks, sims=1, node_capacity=64)
    with pytest.raises(P.AzrError) as e:   # no weights
        eng.validate(rec, batch_size=bs)
    assert e.value.code == AZR_E_STATE
    eng.set_weights(T.make_net_flat(blocks, seed=5))
    with pytest.raises(P.AzrError) as e:   # batch_size < 2
        eng.validate(rec, batch_size=1)
    assert e.value.code == AZR_E_INVALID_ARGUMENT
    lp, lv = eng.validate(rec[:bs - 1], batch_size=bs)   # fewer records than a batch: the reference's 0 / 0, nothing launched
    assert np.isnan(lp) and np.isnan(lv)
    full = eng.validate(rec, batch_size=bs, per_record=True)          # the remainder of 5 is dropped
    exact = eng.validate(rec[:2 * bs], batch_size=bs, per_record=True)
    assert full[:2] == exact[:2] and full[2].tobytes() == exact[2].tobytes() and len(full[2]) == 2 * bs
    eng.close()
