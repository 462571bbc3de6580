"""Host: the per-tile source boxes of the staged undistortion experiment (tools/experiments/undistort_staged.py) hold
every tap of their tile, and tiles that need the border are left to the global path."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "experiments"))
import undistort_staged as staged  # noqa: E402
import undistort_twin as twin  # noqa: E402

SMALL = dict(model="radtan", K=[48, 47, 30.2, 21.7], dist=(-0.25, 0.06, 0.001, -0.002), wh=(61, 45))
EUROC = dict(model="radtan", K=[458.654, 457.296, 367.215, 248.375], dist=(-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05),
             wh=(752, 480))


@pytest.mark.parametrize("spec, K_new, out_wh", [(SMALL, [48, 47, 30.2, 21.7], (61, 45)), (SMALL, [36.0, 35.0, 29.0, 23.0], (61, 45)),
                                                 (SMALL, [30.0, 31.0, 17.5, 14.2], (37, 29)), (EUROC, [356.017, 418.236, 362.992, 250.272], (752, 480))],
                         ids=["small-same", "small-wide", "small-37x29", "euroc-inner"])
def test_boxes_hold_every_tap_of_their_tile(spec, K_new, out_wh):
    ws, hs = spec["wh"]
    tab = twin.table(spec["model"], spec["K"], spec["dist"], K_new, out_wh)
    boxes = staged.tile_boxes(tab, hs, ws)
    tx, ty = -(-out_wh[0] // staged.TILE_W), -(-out_wh[1] // staged.TILE_H)
    assert boxes.shape == (tx * ty, 4) and boxes.dtype == np.int32
    inside = twin.taps_inside(tab, hs, ws)
    ix, iy = tab[..., 0].astype(np.int64) >> 8, tab[..., 1].astype(np.int64) >> 8
    for t, (x0, y0, w, h) in enumerate(boxes):
        rows = slice((t // tx) * staged.TILE_H, (t // tx + 1) * staged.TILE_H)
        cols = slice((t % tx) * staged.TILE_W, (t % tx + 1) * staged.TILE_W)
        if not inside[rows, cols].all():
            assert (x0, y0, w, h) == (0, 0, 0, 0)
            continue
        assert x0 >= 0 and y0 >= 0 and x0 + w <= ws and y0 + h <= hs
        # tight: the first and last tap column / row of the tile
        assert ix[rows, cols].min() == x0 and ix[rows, cols].max() + 2 == x0 + w
        assert iy[rows, cols].min() == y0 and iy[rows, cols].max() + 2 == y0 + h


def test_a_sentinel_empties_its_tile_only():
    tab = twin.table(SMALL["model"], SMALL["K"], SMALL["dist"], SMALL["K"], (128, 8)).copy()
    tab[5, 70] = twin.SENTINEL
    boxes = staged.tile_boxes(tab, 4000, 4000).reshape(2, 2, 4)
    assert (boxes[1, 1] == 0).all() and (boxes[0] != 0).any() and boxes[1, 0, 2] >= 2
    assert 0.0 < staged.staged_share(boxes.reshape(-1, 4)) < 1.0
