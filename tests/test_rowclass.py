"""CPU: the border-class row orders of the tower / training conv tiles (csrc/azr_rowclass.hpp), checked from the header
itself (its constexpr functions compiled for the host): every cell has its own row, pad rows are where pad_from says,
a (tile, tap) pair is marked "skip" only if no cell of the tile has an in-board source under that tap — and every pair
that could be skipped is (the counts DESIGN.md quotes: 9 of 54, 12 of 72, 18 of 99); and the (tap, row) -> source-row table the kernels
build from the header's per-element rules names the neighbouring cell's row of the same board, or the zero row."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """the probe, compiled once"""
    exe = str(tmp_path_factory.mktemp("rowclass") / "rowclass_probe")
    subprocess.check_call([HIPCC, "-O1", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "alphazero-risk_amd", "csrc"),
                           os.path.join(ROOT, "tests", "helpers", "rowclass_probe.hip"), "-o", exe], stderr=subprocess.DEVNULL)
    return exe


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_row_orders_and_skip_masks(probe):
    expect_skips = {2: 9, 3: 12, 4: 18}
    for line in subprocess.check_output([probe]).decode().strip().split("\n"):
        head, rows, skips, pads = [[int(x) for x in part.split()] for part in line.split("|")]
        nb, mt = head
        assert len(rows) == 42 * nb and len(skips) == 9 and len(pads) == mt
        cell_of = {}
        for i, r in enumerate(rows):
            assert 0 <= r < 16 * mt and r not in cell_of, (nb, i, r)
            cell_of[r] = i % 42
        for t in range(mt):      # pad rows close a tile
            for c in range(16):
                assert ((16 * t + c) in cell_of) == (c < pads[t]), (nb, t, c)
        total = 0
        for tap in range(9):
            dy, dx = tap // 3 - 1, tap % 3 - 1
            for t in range(mt):
                cells = [cell_of[r] for r in range(16 * t, 16 * t + 16) if r in cell_of]
                all_out = all(not (0 <= p // 6 + dy < 7 and 0 <= p % 6 + dx < 6) for p in cells)
                marked = bool((skips[tap] >> t) & 1)
                assert marked == all_out, (nb, tap, t)
                total += marked
        assert total == expect_skips[nb], (nb, total)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_source_row_table(probe):
    lines = subprocess.check_output([probe, "taprow"]).decode().strip().split("\n")
    assert len(lines) == 3
    for line in lines:
        head, rows, _, _, table = [[int(x) for x in part.split()] for part in line.split("|")]
        nb, mt = head
        zr = 16 * mt
        assert len(table) == 10 * zr
        cell_of = {r: i for i, r in enumerate(rows)}      # row -> board * 42 + pos
        for tap in range(10):
            dy, dx = tap // 3 - 1, tap % 3 - 1
            for r in range(zr):
                src = table[tap * zr + r]
                if tap == 9 or r not in cell_of:          # all of tap 9, every pad row
                    assert src == zr, (nb, tap, r, src)
                    continue
                b, pos = divmod(cell_of[r], 42)
                y, x = pos // 6 + dy, pos % 6 + dx
                if not (0 <= y < 7 and 0 <= x < 6):       # the tap leaves the board
                    assert src == zr, (nb, tap, r, src)
                    continue
                # a real row under an in-board tap: the row of the neighbouring cell — of the same board
                assert src == rows[b * 42 + y * 6 + x], (nb, tap, r, src)
                assert cell_of[src] // 42 == b, (nb, tap, r, src)
