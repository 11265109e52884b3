"""A Gumbel self-play and its host-stepped retrace (TEST INFRASTRUCTURE, not collected): selfplay_retrace's late golden games played in
device self-play under azr_selfplay_set_gumbel (and azr_selfplay_set_gumbel_tree), and the same games retraced decision by decision
through azr_debug_root_gumbel -> azr_mcts_set_root_gumbel -> azr_mcts_simulate -> azr_mcts_gumbel_policy / _pick.  What a Run gave
is computed once per process; callers must not write into it."""
import numpy as np

import selfplay_retrace as SR

f32 = np.float32
CV, CS, GSEED = 50.0, 0.5, 4242
_cache = {}


def retrace(run, m, tree):
    """SR.retrace's loop for a Gumbel self-play with m root moves, `tree`: the selection below the root.  Per decision the root's vector
    of the draw, one search, gumbel_policy into the record, gumbel_pick as the move.
    ([SR.Game], totals, the games' RNG streams after their last move)"""
    key = ("retrace", run._replace(surprise=None, value_mix=None), m, tree)
    if key in _cache:
        return _cache[key]
    eng = SR.engine(run.threads, run.sims, net=run.net)
    eng.set_gumbel(m, CV, CS)
    eng.set_gumbel_tree(tree)
    states, rngs = SR.late_positions()
    thr = eng.settings.temperature_threshold
    games, streams, tot = [], [], dict(decisions=0, simulations=0, samples=0)
    for g in range(run.quota):
        eng.set_states(np.repeat(states[g:g + 1], SR.G, 0))
        eng.set_rng(np.full(SR.G, rngs[g], np.uint32))
        eng.mcts_clear()
        rows, d = [], 0
        while True:
            valid = eng.valid_moves()
            st = eng.get_states()[0]
            greedy = int(st[144]) + 256 * int(st[145]) > thr
            gum = eng.debug_root_gumbel(GSEED, [run.base + g], [d], valid[:1], [greedy])
            eng.set_root_gumbel(np.repeat(gum, SR.G, 0))
            eng.simulate()
            n, q, prior = (a[0] for a in eng.root_stats())
            pi = eng.gumbel_policy()[0][0]
            mv = eng.gumbel_pick()
            rec = np.zeros(265, np.uint8)
            rec[0] = st[146]
            rec[1:89] = eng.encode()[0]
            rec[93:265] = pi.view(np.uint8)
            rows.append((rec, valid[0], n, q, prior))
            assert (eng.make_moves(mv) == 0).all()
            d += 1; tot["decisions"] += 1; tot["simulations"] += run.sims - run.sims % run.threads; tot["samples"] += 1
            status = int(eng.status()[0])
            if status != -1:
                break
            assert d < 2000
        streams.append(int(eng.get_rng()[0]))
        z = np.array([SR.outcome_z(status, int(row[0][0])) for row in rows], f32)
        for row, zr in zip(rows, z):
            row[0][89:93] = np.array([zr], f32).view(np.uint8)
        cols = [np.array([row[i] for row in rows], t).reshape(shape) for i, (t, shape) in
                enumerate(((np.uint8, (-1, 265)), (np.uint64, -1), (np.uint32, (-1, 43)), (f32, (-1, 43)), (f32, (-1, 43))))]
        games.append(SR.Game(cols[0], z, *cols[1:]))
    eng.close()
    _cache[key] = (games, tot, streams)
    return _cache[key]


def configure(m, tree):
    """what a device self-play's engine is told before its start"""
    def go(eng):
        eng.selfplay_set_gumbel(m, CV, CS, GSEED)
        eng.selfplay_set_gumbel_tree(tree)
    return go


def selfplay(run, m, tree):
    """(records, counters, the slots' RNG streams when the quota is over)"""
    key = ("selfplay", run, m, tree)
    if key not in _cache:
        eng = SR.selfplay(run, configure(m, tree))
        recs, c = SR.play_out(eng, run.quota, 16, 400)
        _cache[key] = (recs, c, eng.get_rng()[:run.quota].tolist())
        eng.close()
    return _cache[key]
