"""GPU parity of the host-stepped PUCT search on the outputs of a trained net (oracle/azr_oracle.c orc_sharp_eval): one-hot and
two-peak priors, exact zeros, fp32 denormals, rows whose legal priors are all zero, values of exactly +-1.  The other search tests
feed both sides near-uniform, strictly positive priors and unsaturated values; here normalize_prior divides denormals and skips a
zero sum, tree_select compares u == Q over whole rows of ties (the umap order decides, with 2 and 4 search threads the skip /
duplicate path), tree_backup averages exact +-1 and one line is dug deep.  Same driver, same assertions as tests/test_gpu_mcts.py:
N, Q, P, the policy, the move, the next state and the RNG, bit for bit.  The other host-stepped comparisons run once more in this
regime in their own modules, beside the helper each reuses: the tree storage (test_gpu_tree_storage.py) and the root-noise search
against the oracle (test_gpu_root_noise.py) on this stub; the root formula under a noise vector, the forced-playout rule
(test_gpu_forced_playouts.py), the capped self-play against the oracle (test_gpu_playout_cap.py) and the Gumbel root search pass by
pass (test_gpu_gumbel.py) on the sharp net, since those comparisons evaluate with the device net, not with a stub."""
import os

import numpy as np
import pytest

import azr_testlib as T
import rules_settings as RS
from gpu_common import search_decisions

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sims,threads", [(24, 1), (25, 2), (102, 4)])
def test_sharp_search_tree_reuse_and_moves_bit_exact(orc, sims, threads):
    """the roots and decisions of test_search_tree_reuse_and_moves_bit_exact; the oracle's side of the run must lie in the regime
    this module is about (azr_testlib.assert_sharp_regime), so a stub edited back to easy outputs fails here"""
    gold = np.load(os.path.join(T.GOLDEN, "rules_games.npz"))
    census = []
    search_decisions(orc, "orc_sharp_eval", sims, threads, gold["states"][::29][:96], 6 if sims <= 25 else 3, census=census)
    n, q, p = (np.stack(a) for a in zip(*census))
    T.assert_sharp_regime(T.sharp_census(n, q, p))


def test_sharp_search_off_the_defaults_bit_exact(orc):
    """all five rule switches off their defaults (tests/rules_settings.py FIVE), 24 simulations, two search threads, 4 decisions"""
    search_decisions(orc, "orc_sharp_eval", 24, 2, RS.search_roots(48), 4, **RS.FIVE)
