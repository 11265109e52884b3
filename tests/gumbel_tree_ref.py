"""The Gumbel search's selection below the root, restated from include/azr.h in np.float32, operation for operation (TEST
INFRASTRUCTURE): score[a] = pi'[a] - (N[a] + act[a]) / (1 + the sum of N + act over the legal moves), pi' the record's policy of
gumbel_ref on the node's own rows; the move is the legal one with the largest score, the lowest index on ties.

tests/test_gumbel_tree_ref.py checks it against float64, the tracking property and the hand cases on the CPU;
tests/test_gpu_gumbel_tree.py pins the device to it bit for bit."""
import numpy as np

from gumbel_ref import MOVES, _best, bits, policy

f32 = np.float32


def select_tree(N, act, Q, P, vhat, valid, c_visit, c_scale):
    """(move, score [43]) of a node met at path depth >= 1; score is 0 on an illegal move"""
    N, act = np.asarray(N, np.uint32), np.asarray(act, np.uint32)
    ok = bits(valid)
    pi, _ = policy(N, Q, P, vhat, valid, c_visit, c_scale)
    cnt = N.astype(np.int64) + act
    den = f32(f32(1.0) + f32(int(cnt[ok].sum()) & 0xFFFFFFFF))
    score = (pi - (cnt.astype(f32) / den).astype(f32)).astype(f32)
    assert score.dtype == f32 and score.shape == (MOVES,)
    return _best(ok, score), np.where(ok, score, f32(0.0)).astype(f32)


def rows(seed, count, top=8):
    """seeded random rows (N, act, Q, P, vhat, valid): Dirichlet(0.3) priors, a zero prior here and there, random masks (every third
    row all legal), N in 0..top on half the moves, a visit in flight on a tenth of them"""
    rng = np.random.default_rng(seed)
    out = []
    for r in range(count):
        valid = int(rng.integers(1, 1 << 43)) if r % 3 else (1 << 43) - 1
        N = (rng.integers(0, top + 1, 43) * (rng.random(43) < 0.5)).astype(np.uint32)
        act = (rng.random(43) < 0.1).astype(np.uint32)
        P = rng.dirichlet(np.full(43, 0.3)).astype(f32)
        if r % 5 == 0:
            P[rng.integers(0, 43, 5)] = 0.0
        out.append((N, act, rng.uniform(-1, 1, 43).astype(f32), P, f32(rng.uniform(-1, 1)), valid))
    return out


def hand_rows():
    """[(name, row, the move the rule must take)]: the hand cases of tests/test_gumbel_tree_ref.py, which states why each move is it"""
    ALL = (1 << 43) - 1
    z, zf = np.zeros(43, np.uint32), np.zeros(43, f32)
    P = np.full(43, 0.5 / 41, f32)
    P[[7, 30]] = 0.25
    out = [("unvisited: the largest prior, the lowest index on a tie", (z, z, zf, P, f32(0.0), ALL), 7)]
    out.append(("one legal move", (z, z, zf, P, f32(0.3), 1 << 19), 19))
    act = z.copy(); act[7] = 1
    out.append(("a visit in flight counts against its move", (z, act, zf, P, f32(0.0), ALL), 30))
    P0 = P.copy(); P0[7] = 0.0
    out.append(("a zero prior: its logit is ln32 of the smallest float, its pi' next to nothing", (z, z, zf, P0, f32(0.0), ALL), 30))
    # the net thought little of the node (vhat -0.5) and move 5 turned out well (Q 0.5 after 3 visits): v_mix = 0.25, sigma lifts move 5
    # by 26.5 * 0.25 over the others, pi'[5] = e^6.6 / (e^6.6 + 42) = 0.946 > 3/4, so it is taken again ...
    Pu = np.full(43, 1.0 / 43, f32)
    Q = zf.copy(); Q[5] = 0.5
    N = z.copy(); N[5] = 3
    out.append(("a high Q draws the visits", (N, z, Q, Pu, f32(-0.5), ALL), 5))
    # ... and with all of 400 visits on it, v_mix has come up to 0.4975 and pi'[5] is 0.04: the others get their turn, the lowest index first
    N = z.copy(); N[5] = 400
    out.append(("overtaken once its share is spent", (N, z, Q, Pu, f32(-0.5), ALL), 0))
    return out
