"""CPU: the fp32 restatement of forced playouts and policy target pruning (tests/forced_playouts_ref.py) against the properties
include/azr.h's definitions imply, on random root statistics, and against one example worked by hand.  The GPU tests
(tests/test_gpu_forced_playouts.py) compare the device with this restatement bit for bit; these tests keep the restatement honest."""
import numpy as np
import pytest

import forced_playouts_ref as F

f32 = np.float32
EPS, HP = 0.25, 1.1


def random_root(rng, searched=True):
    """root statistics as a search leaves them: a legal mask with >= 2 moves, priors over it, visits on some moves, Q in (-1, 1)"""
    ok = rng.random(43) < rng.uniform(0.1, 1.0)
    ok[rng.choice(43, 2, replace=False)] = True
    valid = sum(1 << int(m) for m in np.nonzero(ok)[0])
    p = rng.random(43) * ok
    Pr = (p / p.sum()).astype(f32)
    e = rng.random(43) ** 4 * ok
    eta = (e / e.sum()).astype(f32)
    N = np.zeros(43, np.uint32)
    if searched:
        N[ok] = rng.integers(0, 12, ok.sum()) * (rng.random(ok.sum()) < 0.6)
    Q = np.where(N > 0, rng.uniform(-1, 1, 43), 0).astype(f32)
    return N, Q, Pr, valid, eta


def index_order():
    raise AssertionError("a tie between random fp32 scores")


@pytest.mark.parametrize("k", [0.0, 1e-30])
def test_a_vanishing_factor_is_the_plain_selection(orc, k):
    rng = np.random.default_rng(11)
    visited = 0
    for _ in range(300):
        N, Q, Pr, valid, eta = random_root(rng)
        order = lambda: F.umap_order(orc, valid)
        assert not F.forced_mask(N, Pr, valid, eta, EPS, k).any()
        assert F.forced_pick(N, Q, Pr, valid, eta, EPS, HP, k, order) == F.puct_pick(N, Q, Pr, valid, eta, EPS, HP, order)
        visited += int((N > 0).any())
    assert visited > 200


def test_forcing_picks_among_the_forced_moves_and_changes_picks():
    rng = np.random.default_rng(12)
    changed = forced_roots = 0
    for _ in range(300):
        N, Q, Pr, valid, eta = random_root(rng)
        m = F.forced_mask(N, Pr, valid, eta, EPS, 8.0)
        got = F.forced_pick(N, Q, Pr, valid, eta, EPS, HP, 8.0, index_order)
        plain = F.puct_pick(N, Q, Pr, valid, eta, EPS, HP, index_order)
        assert F.bits(valid)[got]
        if m.any():
            forced_roots += 1
            assert m[got] and N[got] > 0
            u, _ = F.scores(N, Q, F.noised_prior(Pr, eta, EPS), HP)
            assert u[got] == u[m].max()
        else:
            assert got == plain
        changed += int(got != plain)
    assert forced_roots > 100 and changed > 50, (forced_roots, changed)


def test_an_unsearched_root_forces_nothing():
    rng = np.random.default_rng(13)
    for _ in range(50):
        N, Q, Pr, valid, eta = random_root(rng, searched=False)
        assert not F.forced_mask(N, Pr, valid, eta, EPS, 8.0).any()


@pytest.mark.parametrize("k", [0.5, 2.0, 8.0])
def test_pruning_properties(k):
    rng = np.random.default_rng(14)
    pruned = zeroed = 0
    for _ in range(400):
        N, Q, Pr, valid, eta = random_root(rng)
        ok = F.bits(valid)
        Np = F.prune_counts(N, Q, Pr, valid, eta, EPS, HP, k)
        assert (Np <= N).all()                                    # never raises a count
        assert (Np[~ok] == N[~ok]).all() and (Np[N == 0] == 0).all()
        top = N[ok].max()
        cstar = [m for m in range(43) if ok[m] and N[m] == top][0]
        assert Np[cstar] == N[cstar]                              # never touches c*
        nf = F.forced_counts(N, F.noised_prior(Pr, eta, EPS), k)
        for m in np.nonzero(Np != N)[0]:
            f = F.forced_cap(nf[m])
            if Np[m] == 0:                                        # reduced to one playout within f, then pruned outright
                assert int(N[m]) - 1 <= f, (m, N[m], f)
                zeroed += 1
            else:
                assert int(N[m]) - int(Np[m]) <= f and Np[m] >= 2, (m, N[m], Np[m], f)
            pruned += 1
        pi = F.root_policy(Np, valid)
        assert abs(float(pi.astype(np.float64).sum()) - 1.0) <= 43 * 2.0 ** -24 and (pi[~ok] == 0).all()
    assert pruned > 100 and zeroed > 20, (pruned, zeroed)


def test_pruning_is_the_identity_where_no_move_is_below_the_best():
    """Q = +1 on every move but the most visited one, Q = -1 there: Q[m] + v / n >= 1 > U* = -1 + v* / (1 + N*) as long as
    v* < 2 (1 + N*), which the assert below checks — the PUCT condition holds for no move at any count"""
    rng = np.random.default_rng(15)
    for _ in range(200):
        N, _, Pr, valid, eta = random_root(rng)
        ok = F.bits(valid)
        top = N[ok].max()
        cstar = [m for m in range(43) if ok[m] and N[m] == top][0]
        Q = np.where(np.arange(43) == cstar, -1, 1).astype(f32)
        _, v = F.scores(N, Q, F.noised_prior(Pr, eta, EPS), HP)
        assert v[cstar] < 2 * (1 + int(N[cstar]))
        assert (F.prune_counts(N, Q, Pr, valid, eta, EPS, HP, 8.0) == N).all()


def test_no_factor_prunes_nothing():
    rng = np.random.default_rng(16)
    for _ in range(100):
        N, Q, Pr, valid, eta = random_root(rng)
        assert (F.prune_counts(N, Q, Pr, valid, eta, EPS, HP, 0.0) == N).all()


def test_hand_worked_example():
    """five legal moves, eps = 0 (noiseP = P), hp = 1, k = 2; sumN = 17, sqrt(1 + 17) = 4.2426
         m   N    P      Q      v = P * 4.2426   nf = sqrt(34 P)   f
         0   10   0.5    0.1    2.1213
         1   4    0.25   -0.5   1.0607           2.915             2
         2   2    0.125  0.0    0.5303           2.062             2
         3   1    0.125  -0.2   0.5303           2.062             2
         4   0    0      0      0
    c* = 0, U* = 0.1 + 2.1213 / 11 = 0.2928.
    m = 1: lower = 2.  N' = 4: -0.5 + 1.0607 / 4 = -0.235 < U* -> 3;  -0.5 + 1.0607 / 3 = -0.146 < U* -> 2;  2 is the bound.
    m = 2: lower = 0.  N' = 2: 0.5303 / 2 = 0.265 < U* -> 1;  0.5303 / 1 = 0.530 >= U*: stop at 1 < N -> pruned to 0.
    m = 3: lower = 0.  N' = 1: -0.2 + 0.5303 = 0.330 >= U*: stays 1 (not reduced, so not zeroed).
    m = 4: never visited."""
    N = np.zeros(43, np.uint32); N[:5] = [10, 4, 2, 1, 0]
    Pr = np.zeros(43, f32); Pr[:5] = [0.5, 0.25, 0.125, 0.125, 0.0]
    Q = np.zeros(43, f32); Q[:5] = [0.1, -0.5, 0.0, -0.2, 0.0]
    eta = np.full(43, 0.3, f32)
    Np = F.prune_counts(N, Q, Pr, 0b11111, eta, 0.0, 1.0, 2.0)
    assert list(Np[:5]) == [10, 2, 0, 1, 0] and (Np[5:] == 0).all()
    pi = F.root_policy(Np, 0b11111)
    assert list(pi[:5]) == [f32(10) / f32(13), f32(2) / f32(13), 0, f32(1) / f32(13), 0]
    # the same root as a selection: moves 2 and 3 are tried and short of nf = 2.06, so they are the only candidates, and move 2 scores
    # higher (0 + 0.5303 / 3 = 0.177 against -0.2 + 0.5303 / 2 = 0.065); plain PUCT takes move 0 (0.2928)
    assert list(np.nonzero(F.forced_mask(N, Pr, 0b11111, eta, 0.0, 2.0))[0]) == [2, 3]
    assert F.forced_pick(N, Q, Pr, 0b11111, eta, 0.0, 1.0, 2.0, index_order) == 2
    assert F.puct_pick(N, Q, Pr, 0b11111, eta, 0.0, 1.0, index_order) == 0
