"""CPU: the Gumbel root search as include/azr.h states it, through its np.float32 restatement (tests/gumbel_ref.py): exp32 against the
float64 exponential with the header's measured error as the bound; the considered-visit sequence on the hand example, the degenerate
cases and every (m_eff <= 43, n <= 128) played out; the Gumbel-max property of the draw; the record's policy.  The bounds: exp32's
are the maxima measured on this file's grid (2 000 001 arguments of [-104, 0] and their float neighbours at every integer), asserted
without slack; the draw's is 4 binomial standard deviations per move over 20 000 rows (one failure in 16 000 for a correct sampler,
and the rows are fixed); the policy's sum is 43 roundings of at most one ulp of 1."""
import numpy as np

import gumbel_ref as G

f32 = np.float32
ALL = (1 << 43) - 1


def exp_grid():
    x = -np.linspace(0.0, 104.0, 2_000_001).astype(f32)
    ints = -np.arange(0, 105, dtype=f32)
    return np.unique(np.concatenate([x, ints, np.nextafter(ints, f32(0)), np.nextafter(ints[:-1], f32(-200))]))


def test_exp32_against_the_float64_exponential():
    x = exp_grid()
    assert x.min() == -104 and x.max() == 0
    got, ref = G.exp32(x).astype(np.float64), np.exp(x.astype(np.float64))
    assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
    normal = ref >= 1.17549435e-38
    rel = (np.abs(got - ref)[normal] / ref[normal]).max()
    den = (np.abs(got - ref)[~normal] / 2.0 ** -149).max()
    print("exp32 over %d arguments: max relative error %.4g on normal results, max error %.4g of the smallest denormal below" % (len(x), rel, den))
    assert rel <= G.EXP32_REL and den <= G.EXP32_DENORMAL_ULP
    assert rel > 0.9 * G.EXP32_REL and den > 0.9 * G.EXP32_DENORMAL_ULP     # the header states the measured figure, not a loose one


def test_exp32_exact_cases():
    assert G.exp32(f32(0.0)).tobytes() == f32(1.0).tobytes() and G.exp32(f32(-0.0)).tobytes() == f32(1.0).tobytes()
    far = G.exp32(np.array([-104.0, -104.00001, -150.0, -1e30, -np.inf, -103.0, -87.5], f32))
    assert not np.isnan(far).any() and (far[:5] == 0).all(), far
    assert 0 < far[5] < 1.2e-38 and far[5] == f32(far[5]) and far[6] > 0        # a denormal, no NaN
    assert abs(float(far[5]) - np.exp(-103.0)) <= G.EXP32_DENORMAL_ULP * 2.0 ** -149
    x = -np.linspace(0, 104, 4001).astype(f32)
    assert (np.diff(G.exp32(x).astype(np.float64)) <= 0).all()                  # monotone on a coarse grid


def test_considered_visits_hand_example_and_degenerate_cases():
    assert [G.considered_visit(4, 16, i) for i in range(16)] == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5]
    assert [G.considered_visit(1, 9, i) for i in range(9)] == list(range(9))
    assert [G.considered_visit(0, 5, i) for i in range(5)] == list(range(5))
    assert [G.considered_visit(43, 16, i) for i in range(16)] == [0] * 16           # only 16 of the 43 are ever visited
    assert [G.considered_visit(8, 5, i) for i in range(5)] == [0] * 5               # n < m_eff
    assert [G.considered_visit(2, 7, i) for i in range(7)] == [0, 0, 1, 1, 2, 2, 3]


def _play(m, legal, n, scores_of):
    """the n claims of one search with one thread on static scores: (search-local visits [43], the moves in claim order)"""
    valid = (1 << legal) - 1
    N, moves = np.zeros(43, np.uint32), []
    P = np.full(43, 1.0 / legal, f32)
    for i in range(n):
        mv, cv = G.select(N, np.zeros(43), np.zeros(43), np.zeros(43, f32), P, scores_of, 0.0, valid, i, m, n, 50.0, 0.5)
        assert mv < legal and cv == G.considered_visit(min(m, legal), n, i)
        N[mv] += 1
        moves.append(mv)
    return N, moves


def test_the_hand_example_leaves_6_6_2_2():
    g = np.zeros(43, f32); g[[5, 2, 7, 0]] = [4.0, 3.0, 2.0, 1.0]                   # distinct static scores: Q stays 0
    N, moves = _play(4, 9, 16, g)
    assert moves[:4] == [5, 2, 7, 0] and sorted(N[N > 0].tolist()) == [2, 2, 6, 6] and N[5] == N[2] == 6


def test_every_sequence_spends_the_budget_on_the_top_m():
    rng = np.random.default_rng(5)
    for m_eff in range(1, 44):
        order = rng.permutation(43)
        g = np.zeros(43, f32); g[order] = np.arange(43, 0, -1, dtype=f32)          # distinct: order[0] is the best move
        for n in range(1, 129):
            counts = np.zeros(43, np.int64)
            for i in range(n):                                                       # the selection on static scores, inlined (cheap)
                cv = G.considered_visit(m_eff, n, i)
                at = np.nonzero(counts == cv)[0]
                assert len(at), (m_eff, n, i, cv)                                    # no fallback is ever needed on a fresh root
                counts[at[np.argmax(g[at])]] += 1
            assert counts.sum() == n and (counts[order[m_eff:]] == 0).all(), (m_eff, n, counts)
            assert counts[order[0]] == counts.max()


def test_selection_fallbacks_ties_and_n0():
    P, Q = np.full(43, 0.1, f32), np.zeros(43, f32)
    g = np.zeros(43, f32); g[3], g[4] = 1.0, 1.0
    z = np.zeros(43)
    # a tie: lowest index
    assert G.select(z, z, z, Q, P, g, 0.0, ALL, 0, 4, 16, 50, 0.5) == (3, 0)
    # N0 != 0: search-local counts decide, not N
    N = np.full(43, 7); N0 = N.copy(); N0[9] = 6
    mv, cv = G.select(N, N0, z, Q, P, g, 0.0, ALL, 4, 4, 16, 50, 0.5)                 # cv = 1: only move 9 has ns = 1
    assert (mv, cv) == (9, 1)
    # first fallback: nobody at cv = 2, the largest count below it wins over a better score at a smaller count
    N = np.zeros(43); N[[3, 20]] = [0, 1]
    assert G.select(N, z, z, Q, P, g, 0.0, ALL, 8, 4, 16, 50, 0.5) == (20, 2)
    # second fallback: everybody is above cv
    assert G.select(np.full(43, 5), z, z, Q, P, g, 0.0, ALL, 0, 4, 16, 50, 0.5) == (3, 0)
    # in-flight visits count
    act = np.zeros(43); act[3] = 1
    assert G.select(z, z, act, Q, P, g, 0.0, ALL, 1, 4, 16, 50, 0.5) == (4, 0)


def test_gumbel_max_samples_the_prior():
    prior = np.array([0.5, 0.25, 0.15, 0.07, 0.03], f32)
    lg = G.logit(prior)
    rows, hits = 20000, np.zeros(5, np.int64)
    for r in range(rows):
        g = G.draw(1234, 1000 + r % 200, r // 200, 0b11111)
        assert not g[5:].any()
        hits[int(np.argmax(g[:5] + lg))] += 1
    p = prior.astype(np.float64) / prior.astype(np.float64).sum()
    dev = np.abs(hits - rows * p) / np.sqrt(rows * p * (1 - p))
    print("argmax frequencies", hits / rows, "prior", p, "deviations in sigma", dev)
    assert (dev <= 4).all(), dev
    assert not G.draw(1234, 1000, 0, 0b11111, greedy=True).any()


def test_policy_sums_to_one_and_respects_the_mask():
    rng = np.random.default_rng(9)
    for trial in range(200):
        valid = int(rng.integers(1, 1 << 43)) if trial else ALL
        ok = G.bits(valid)
        P = rng.dirichlet(np.full(43, 0.3)).astype(f32)
        N = (rng.integers(0, 30, 43) * (rng.random(43) < 0.4)).astype(np.uint32)
        Q = rng.uniform(-1, 1, 43).astype(f32)
        pi, qhat = G.policy(N, Q, P, f32(rng.uniform(-1, 1)), valid, 50.0, float(rng.choice([0.05, 0.5, 1.0])))
        assert not pi[~ok].any() and (pi[ok] >= 0).all() and not np.isnan(pi).any()
        assert abs(float(pi.astype(np.float64).sum()) - 1.0) <= 43 * 2.0 ** -24, pi.sum()
        assert (qhat[ok & (N > 0)] == Q[ok & (N > 0)]).all()
    pi, _ = G.policy(np.zeros(43), np.zeros(43, f32), np.full(43, 1 / 43, f32), 0.3, 1 << 17, 50.0, 0.5)
    assert pi[17].tobytes() == f32(1.0).tobytes() and pi.sum() == 1.0


def test_completed_q_and_the_move():
    P = np.array([0.5, 0.3, 0.2] + [0.0] * 40, f32)
    N = np.array([3, 0, 1] + [0] * 40, np.uint32)
    Q = np.array([0.5, 0.9, -0.5] + [0.0] * 40, f32)
    qhat, v_mix = G.completed_q(N, Q, P, 0.1, 0b111)
    want = (0.1 + 4 * ((0.5 * 0.5 + 0.2 * -0.5) / 0.7)) / 5
    assert abs(float(v_mix) - want) < 1e-6 and qhat[1] == v_mix and qhat[0] == Q[0] and qhat[2] == Q[2]
    assert G.completed_q(np.zeros(43), Q, P, 0.1, 0b111)[1] == f32(0.1)              # nothing visited: v_mix = vhat
    g = np.zeros(43, f32)
    assert G.move([3, 3, 1] + [0] * 40, np.zeros(43), Q, P, g, 0.1, 0b111, 50, 0.5) == 1      # most visited, then the score (Q 0.9)
    assert G.move([9, 3, 1] + [0] * 40, [8, 0, 0] + [0] * 40, Q, P, g, 0.1, 0b111, 50, 0.5) == 1   # search-local counts
