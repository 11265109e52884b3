"""GPU parity of the tree STORAGE (csrc/azr_tree.hpp): the node pool with its free stack, the open-addressing table with 16-bit tags
probed 16 slots at a time, and the trim that rebuilds the table.  The search tests run on a roomy pool and a table that hardly ever
collides; here the pool is exactly full, too short, and the table is made to collide.

Every case is a host-stepped search with the oracle's stub net (orc_hash_eval: no network involved) over the golden roots, six decisions
with tree reuse, sampling on odd steps, compared with the oracle per decision and game bit for bit: N, Q, P, the policy, the picked
move, the next state and the RNG (azr_testlib.engine_matches_tree_run).  A search gets S + 8 passes: one that does not finish fails.
  * exact fit: node_capacity = the unbounded oracle's peak node count — hiwater reaches C, the free stack is recycled through five
    trims, nothing is dropped;
  * short pool: node_capacity 8 and 16 against the oracle's bounded store (orc_mcts_set_node_limit, tests/test_oracle_node_limit.py):
    the dropped leaf, the root that finds the pool full and empties the tree, and nodes_dropped equal to the oracle's count;
  * colliding table (libazr_hip_test.so, AZR_TREE_HASH_AND / AZR_TREE_HASH_OR): one chain with equal tags, one start slot, one tag,
    chains that wrap round the table's end — placement must never change what a search returns;
  * device self-play and the two-net arena (tree 2, tree_trim_twice, the game turnover) on the one-chain table against the product
    library, byte for byte."""
import numpy as np
import pytest

import azr_testlib as T
from gpu_common import pkg

pytestmark = pytest.mark.gpu

SHAPES = [(24, 1), (25, 2), (42, 4)]
# (AZR_TREE_HASH_AND, AZR_TREE_HASH_OR): key_hash returns (h & AND) | OR
HASHES = {"one_chain_equal_tags": (0, 1), "one_start_slot": (0xffff0000, 0), "one_tag": (0x0000ffff, 0),
          "wrapping_chains": (0xffff0003, 0xfffc)}


def run_engine(run, monkeypatch=None, hash_hook=None, **kw):
    """the recorded oracle run `run` played on a fresh engine; returns its counters"""
    P = pkg()
    if hash_hook:
        monkeypatch.setenv("AZR_TREE_HASH_AND", hex(hash_hook[0]))
        monkeypatch.setenv("AZR_TREE_HASH_OR", hex(hash_hook[1]))
    eng = P.Engine(run["G"], blocks=1, sims=run["sims"], dtype=P.NET_F32, threads=run["threads"], test_hooks=bool(hash_hook), **kw)
    if hash_hook:
        monkeypatch.delenv("AZR_TREE_HASH_AND")
        monkeypatch.delenv("AZR_TREE_HASH_OR")
    try:
        T.engine_matches_tree_run(eng, run)
        c = eng.counters()
    finally:
        eng.close()
    assert c["errors"] == 0
    assert c["simulations"] == int(run["alive"].sum()) * (run["sims"] - run["sims"] % run["threads"])
    return c


@pytest.mark.parametrize("sims,threads", SHAPES)
def test_pool_that_fits_exactly(orc, sims, threads):
    """node_capacity = the peak node count of the unbounded oracle: the pool fills to its last node (hiwater == C) and is refilled from
    the free stack after every trim; results are the unbounded oracle's and nothing is dropped"""
    run = T.orc_tree_run(sims, threads)
    assert 8 < run["peak"] < 16 * (sims + 1)
    c = run_engine(run, node_capacity=run["peak"])
    assert c["nodes_dropped"] == 0


@pytest.mark.parametrize("unvisited", [False, True], ids=["picked", "unvisited"])
@pytest.mark.parametrize("capacity", [8, 16])
@pytest.mark.parametrize("sims,threads", SHAPES)
def test_short_pool(orc, sims, threads, capacity, unvisited):
    """a pool of 8 / 16 nodes against the oracle's store with the same limit: leaves that are not stored (asked for again by later
    descents, their values backed up) and roots that find the pool full after the trim and empty the tree.  `unvisited` plays the
    lowest legal move the search never tried where there is one, so that the next root is (mostly) not in the tree.  The path stack
    is min(C, 1024) = 8 or 16 deep here: AZR_E_CAPACITY would show as an error."""
    run = T.orc_tree_run(sims, threads, limit=capacity, unvisited=unvisited)
    assert run["dropped"] > 0 and run["evictions"] > 0   # (the oracle alone: the comparison below is not vacuous)
    c = run_engine(run, node_capacity=capacity)
    assert c["nodes_dropped"] == run["dropped"]


@pytest.mark.parametrize("capacity", [0, 16], ids=["default_pool", "pool16"])
@pytest.mark.parametrize("sims,threads", SHAPES[:2])
@pytest.mark.parametrize("name", list(HASHES))
def test_colliding_table(orc, monkeypatch, name, sims, threads, capacity):
    """the table made to collide (every second golden root): the results are those of the same oracle runs as above"""
    run = T.orc_tree_run(sims, threads, limit=capacity, stride=2)
    c = run_engine(run, monkeypatch, HASHES[name], node_capacity=capacity)
    assert c["nodes_dropped"] == run["dropped"]
    if capacity:
        assert run["dropped"] > 0 and run["evictions"] > 0


# ---- the same pools on the sharp stub (orc_sharp_eval): one-hot priors and values of +-1 dig one line deep instead of spreading ----------
SHARP = "orc_sharp_eval"


@pytest.mark.parametrize("sims,threads", SHAPES)
def test_sharp_pool_that_fits_exactly(orc, sims, threads):
    run = T.orc_tree_run(sims, threads, stub=SHARP)
    assert 8 < run["peak"] < 16 * (sims + 1)
    c = run_engine(run, node_capacity=run["peak"])
    assert c["nodes_dropped"] == 0


@pytest.mark.parametrize("capacity", [8, 16])
@pytest.mark.parametrize("sims,threads", SHAPES)
def test_sharp_short_pool(orc, sims, threads, capacity):
    """the path stack is min(C, 1024) = 8 or 16 deep and the sharp stub's lines are the deepest the suite searches: AZR_E_CAPACITY
    where the oracle plays on would show as an error"""
    run = T.orc_tree_run(sims, threads, limit=capacity, stub=SHARP)
    assert run["dropped"] > 0 and run["evictions"] > 0
    c = run_engine(run, node_capacity=capacity)
    assert c["nodes_dropped"] == run["dropped"]


@pytest.mark.parametrize("capacity", [0, 16], ids=["default_pool", "pool16"])
@pytest.mark.parametrize("name", ["one_chain_equal_tags", "wrapping_chains"])
def test_sharp_colliding_table(orc, monkeypatch, name, capacity):
    run = T.orc_tree_run(25, 2, limit=capacity, stride=2, stub=SHARP)
    c = run_engine(run, monkeypatch, HASHES[name], node_capacity=capacity)
    assert c["nodes_dropped"] == run["dropped"]
    if capacity:
        assert run["dropped"] > 0 and run["evictions"] > 0


def test_selfplay_and_arena_on_the_one_chain_table(monkeypatch):
    """device self-play (24 games on 16 slots: the game turnover) and the two-net concurrent-mirror arena (tree 2, the two trims in a
    row at a turn's first decision) with every key in one chain of equal tags: records in canonical order and arena results are the
    product library's, byte for byte"""
    P = pkg()
    out = {}
    for hook in (False, True):
        if hook:
            monkeypatch.setenv("AZR_TREE_HASH_AND", "0")
            monkeypatch.setenv("AZR_TREE_HASH_OR", "1")
        a = P.Engine(16, blocks=1, sims=8, dtype=P.NET_BF16, threads=2, max_game_rounds=12, test_hooks=hook)
        b = P.Engine(16, blocks=1, sims=8, dtype=P.NET_BF16, threads=2, max_game_rounds=12, test_hooks=hook)
        if hook:
            monkeypatch.delenv("AZR_TREE_HASH_AND")
            monkeypatch.delenv("AZR_TREE_HASH_OR")
        a.set_weights(T.make_net_flat(1, seed=31, perturb_bn=True))
        b.set_weights(T.make_net_flat(1, seed=32, perturb_bn=True))
        a.selfplay_start_games(4242, 24)
        for _ in range(400):
            if a.counters()["games_finished"] >= 24:
                break
            a.selfplay_run(64)
        else:
            raise AssertionError("self-play did not finish")
        recs = a.drain()
        a.arena_set_opponent(b)
        a.arena_collect_samples(True)
        a.arena_start(P.PLAYER_ALPHAZERO, P.PLAYER_ALPHAZERO_B, 16, 0, P.MIRROR_CONCURRENT, 99)
        for _ in range(4000):
            if a.arena_run(64):
                break
        else:
            raise AssertionError("arena did not finish")
        canon = lambda r: np.sort(np.ascontiguousarray(r).view("S265").ravel()).tobytes()   # noqa: E731  (games finish in any order within a pass)
        c = a.counters()
        out[hook] = (canon(recs), a.arena_results(), canon(a.drain()), c["nodes_dropped"], c["errors"])
        a.arena_set_opponent(None)
        a.close(); b.close()
    assert len(out[False][0]) > 0 and len(out[False][2]) > 0
    assert out[False][3:] == (0, 0)
    assert out[False] == out[True]
