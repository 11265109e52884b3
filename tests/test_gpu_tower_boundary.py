"""GPU parity across the layer boundary of the single-image tower tiles (k_tower_sb<NB>, csrc/azr_tower_sb.hip): the folded BN
scale / shift of each layer handed to the epilogue through LDS, the residual operand of every row tile kept in registers and updated
in place by the shortcut layers.  None of it may change a bit: every tile shape is compared with the independently written one-board
kernel (k_tower_bf16<1>, AZR_TOWER_SB=0)."""
import functools
import os

import numpy as np
import pytest

import azr_testlib as T
from gpu_common import pkg

pytestmark = pytest.mark.gpu

N_MAX = 13
SIZES = (4, 5, 13)   # boards per launch: one full 4-board workgroup, a partly filled last one, several


@functools.lru_cache(maxsize=None)
def inputs():
    g = np.unique(np.load(os.path.join(T.GOLDEN, "encode.npz"))["in88"], axis=0)   # distinct rows
    x = g[np.linspace(0, len(g) - 1, N_MAX).astype(int)].copy()
    assert len(np.unique(x, axis=0)) == N_MAX
    x.setflags(write=False)
    return x


def forward(mode, dtype_name, blocks):
    """pi, v for each launch size, through the test-hook library with AZR_TOWER_SB=mode (read once, at engine creation)"""
    P = pkg()
    old = os.environ.get("AZR_TOWER_SB")
    os.environ["AZR_TOWER_SB"] = mode
    try:
        eng = P.Engine(N_MAX, blocks=blocks, sims=1, dtype=getattr(P, dtype_name), node_capacity=64, test_hooks=True)
    finally:
        if old is None:
            del os.environ["AZR_TOWER_SB"]
        else:
            os.environ["AZR_TOWER_SB"] = old
    eng.set_weights(T.make_net_flat(blocks, seed=3, perturb_bn=True))   # perturbed BN: a scale or shift of the wrong layer or channel changes bits
    out = {n: eng.predict(inputs()[:n].copy()) for n in SIZES}
    eng.close()
    return out


@functools.lru_cache(maxsize=None)
def reference(dtype_name, blocks):
    """the one-board two-image kernel: computed once per net, shared by the tile shapes, never modified"""
    out = forward("0", dtype_name, blocks)
    for pi, v in out.values():
        pi.setflags(write=False)
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("mode", ["2", "4", "3"], ids=["4-board", "3-board", "2-board"])
@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("dtype_name", ["NET_BF16", "NET_F16"])
def test_tile_boundary_bit_identical(dtype_name, blocks, mode):
    """blocks = 1: the first and the last layer are the only block, the residual comes straight from the stem; blocks = 3: both
    parities more than once, each layer with its own folded BN values, and a residual written by a shortcut layer and consumed
    by the next block.  pi and v of the forced tile equal the one-board kernel's bit for bit at every launch size."""
    ref = reference(dtype_name, blocks)
    out = forward(mode, dtype_name, blocks)
    for n in SIZES:
        pi, v = out[n]
        rpi, rv = ref[n]
        assert pi.shape == rpi.shape == (n, 43) and v.shape == rv.shape == (n,)
        assert np.isfinite(pi).all() and np.isfinite(v).all()
        assert (pi.view(np.uint32) == rpi.view(np.uint32)).all(), (dtype_name, blocks, mode, n)
        assert (v.view(np.uint32) == rv.view(np.uint32)).all(), (dtype_name, blocks, mode, n)
    # distinct boards give distinct outputs: a tile that answered every board with one board's values would not pass as "equal"
    assert len(np.unique(ref[N_MAX][0], axis=0)) == N_MAX
