"""The oracle's bounded node store (orc_mcts_set_node_limit, oracle/azr_oracle.h): the engine's node pool restated, which the GPU tree
storage tests (test_gpu_tree_storage.py) compare a full and a short pool with.  CPU only.
  * a limit that is never exceeded changes nothing: with limit = the unbounded run's peak node count, N, Q, P, the policies, the moves,
    the next states and the RNG streams of six decisions over the 96 golden roots are the unbounded run's, and nothing is dropped;
  * a limit of 8 never stops a search: every one completes S - S % T simulations;
  * on these inputs both the drop (a) and the eviction (b) happen, so a comparison with this oracle is not vacuous."""
import pytest

import azr_testlib as T

SHAPES = [(24, 1), (25, 2), (42, 4)]
FIELDS = ("alive", "n", "q", "p", "pi", "picked", "played", "after", "rng")


@pytest.mark.parametrize("sims,threads", SHAPES)
def test_limit_at_the_peak_changes_nothing(orc, sims, threads):
    free = T.orc_tree_run(sims, threads)
    assert free["dropped"] == 0 and free["evictions"] == 0 and 8 < free["peak"] < 16 * (sims + 1)
    fit = T.orc_tree_run(sims, threads, limit=free["peak"])
    for f in FIELDS:
        assert free[f].tobytes() == fit[f].tobytes(), f
    assert fit["dropped"] == 0 and fit["evictions"] == 0 and fit["peak"] == free["peak"]


@pytest.mark.parametrize("unvisited", [False, True])
@pytest.mark.parametrize("limit", [8, 16])
@pytest.mark.parametrize("sims,threads", SHAPES)
def test_short_store_ends_every_search_and_drops(orc, sims, threads, limit, unvisited):
    run = T.orc_tree_run(sims, threads, limit=limit, unvisited=unvisited)
    assert run["alive"][0].all()
    assert run["sims_per_search"] == {sims - sims % threads}
    assert run["peak"] == limit
    assert run["dropped"] > 0 and run["evictions"] > 0
    # every eviction empties a full store
    assert run["dropped"] >= limit * run["evictions"]
