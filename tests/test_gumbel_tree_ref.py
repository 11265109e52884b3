"""CPU: the restatement of the Gumbel search's selection below the root (tests/gumbel_tree_ref.py) against the same rule in float64,
the property that makes it "visits proportional to pi'", and the hand cases."""
import numpy as np

import gumbel_ref as G
import gumbel_tree_ref as GT

f32 = np.float32
CV, CS = 50.0, 0.5
ALL = (1 << 43) - 1


def _scores64(N, act, Q, P, vhat, valid, c_visit=CV, c_scale=CS):
    """the header's rule with every float operation in float64 and the library's log and exp; -inf on an illegal move"""
    N, act, Q, P = (np.asarray(a, np.float64) for a in (N, act, Q, P))
    ok = G.bits(valid)
    seen = ok & (N > 0)
    total = N[ok].sum()
    wp, wq = P[seen].sum(), (P[seen] * Q[seen]).sum()
    v_mix = (float(vhat) + total * (wq / wp)) / (1.0 + total) if total > 0 and wp > 0 else float(vhat)
    qhat = np.where(seen, Q, v_mix)
    x = np.log(np.maximum(P, float(np.float32(1.17549435e-38)))) + (c_visit + N[ok].max()) * c_scale * qhat
    e = np.where(ok, np.exp(x - x[ok].max()), 0.0)
    cnt = N + act
    return np.where(ok, e / e.sum() - cnt / (1.0 + cnt[ok].sum()), -np.inf)


def test_the_float32_rule_picks_the_float64_move():
    rows = GT.rows(11, 600)
    left_out, moves = 0, set()
    for r, (N, act, Q, P, vhat, valid) in enumerate(rows):
        s64 = _scores64(N, act, Q, P, vhat, valid)
        top = np.sort(s64[np.isfinite(s64)])[::-1]
        mv, score = GT.select_tree(N, act, Q, P, vhat, valid, CV, CS)
        assert np.isfinite(score).all() and not score[~G.bits(valid)].any()
        if len(top) > 1 and top[0] - top[1] < 1e-6:
            left_out += 1
            continue
        assert mv == int(np.argmax(s64)), (r, mv, int(np.argmax(s64)), top[:2])
        moves.add(mv)
    print("rows left out for a margin below 1e-6: %d of %d; distinct moves taken: %d" % (left_out, len(rows), len(moves)))
    assert left_out <= 0.02 * len(rows) and len(moves) > 20


def test_frozen_policy_visits_track_the_policy():
    """Q = 0 and vhat = 0 make pi' the softmax of the logits whatever the counts are: applied n = 1..128 times from empty counts, the
    rule keeps every N[a] within one visit of n * pi'[a]"""
    rng = np.random.default_rng(5)
    worst = 0.0
    for case in range(50):
        P = rng.dirichlet(np.full(43, 0.3)).astype(f32)
        valid = ALL if case % 2 else int(rng.integers(1, 1 << 43))
        N, z = np.zeros(43, np.uint32), np.zeros(43, f32)
        pi = G.policy(N, z, P, 0.0, valid, CV, CS)[0].astype(np.float64)
        for n in range(1, 129):
            mv, _ = GT.select_tree(N, np.zeros(43, np.uint32), z, P, 0.0, valid, CV, CS)
            assert G.bits(valid)[mv]
            N[mv] += 1
            assert G.policy(N, z, P, 0.0, valid, CV, CS)[0].tobytes() == pi.astype(f32).tobytes()   # frozen indeed
            worst = max(worst, float(np.abs(N - n * pi).max()))
            assert worst < 1.0, (case, n, worst)
    print("max |N(a) - n pi'(a)| over 50 priors and n <= 128: %.3f" % worst)


def test_hand_cases():
    for name, row, want in GT.hand_rows():
        mv, score = GT.select_tree(*row, CV, CS)
        assert mv == want, (name, mv, want, score)
    by_name = {name.split(":")[0]: row for name, row, _ in GT.hand_rows()}
    # unvisited and Q = vhat = 0: the scores are pi' = the prior over its 43-term sum
    N, act, Q, P, vhat, valid = by_name["unvisited"]
    score = GT.select_tree(N, act, Q, P, vhat, valid, CV, CS)[1]
    assert score[7] == score[30] == score.max() and np.abs(score - P).max() < 1e-6
    # one legal move: pi' = 1 on it, nothing is subtracted
    assert GT.select_tree(*by_name["one legal move"], CV, CS)[1][19] == 1.0
    # the visit in flight: half of 1 + 1 goes off move 7's score
    row = by_name["a visit in flight counts against its move"]
    score = GT.select_tree(*row, CV, CS)[1]
    pi = G.policy(row[0], *row[2:], CV, CS)[0]
    assert score[7] == f32(pi[7] - f32(0.5)) and score[30] == pi[30] and abs(float(score[7]) + 0.25) < 1e-6
    # the zero prior: a number, below every other move's, and not negative
    score = GT.select_tree(*by_name["a zero prior"], CV, CS)[1]
    assert 0.0 <= score[7] < 1e-30 and (np.delete(score, 7) > 1e-3).all()


def test_a_high_q_is_overtaken_once_its_share_is_spent():
    """the hand row with a high Q on move 5, played on with the Q row held still: move 5 is taken first, and the first other move comes
    in exactly when move 5's share of the visits has reached its pi' (less the newcomer's own pi', which is what the rule compares)"""
    (N, act, Q, P, vhat, valid) = next(row for name, row, _ in GT.hand_rows() if name.startswith("a high Q"))
    N, taken = N.copy(), []
    for n in range(40):
        mv, _ = GT.select_tree(N, act, Q, P, vhat, valid, CV, CS)
        pi = G.policy(N, Q, P, vhat, valid, CV, CS)[0].astype(np.float64)
        share = N[5] / (1.0 + N.sum())
        if mv == 5:
            assert share < pi[5], (n, share, pi[5])
        else:
            assert N[mv] == 0 and share > pi[5] - pi[mv] - 1e-6, (n, mv, share, pi[5], pi[mv])
        taken.append(mv)
        N[mv] += 1
    print("moves taken:", taken)
    assert taken[0] == 5 and taken.count(5) > 20 and set(taken) != {5}
