"""GPU: the staged undistortion experiment (tools/experiments/undistort_staged.hip) gives the bytes of
tests/undistort_twin.py, the same as the library's kernel, on tiles it stages, on tiles it leaves to the global path and
with boxes that do not belong to the table."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "experiments"))
import undistort_staged as staged  # noqa: E402
import undistort_twin as twin  # noqa: E402

pytestmark = pytest.mark.gpu

RADTAN = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)
SMALL = dict(model="radtan", K=[48, 47, 30.2, 21.7], dist=(-0.25, 0.06, 0.001, -0.002), wh=(61, 45))
EUROC = dict(model="radtan", K=[458.654, 457.296, 367.215, 248.375], dist=RADTAN, wh=(752, 480))
HD = dict(model="radtan", K=[458.654 * 1920 / 752, 457.296 * 1080 / 480, 367.215 * 1920 / 752, 248.375 * 1080 / 480], dist=RADTAN,
          wh=(1920, 1080))
# spec, K_new, out (W, H): tiles wholly staged, tiles with outside taps, Wo % 4 != 0 and a row pitch off 16 bytes, more
# than one tile each way, and the size the A/B is run at ("inner" of tests/test_camera_host.py, scaled for HD)
CASES = {
    "small-same": (SMALL, [48, 47, 30.2, 21.7], (61, 45)),
    "small-wide": (SMALL, [36.0, 35.0, 29.0, 23.0], (61, 45)),
    "small-37x29": (SMALL, [30.0, 31.0, 17.5, 14.2], (37, 29)),
    "euroc-inner": (EUROC, [356.017, 418.236, 362.992, 250.272], (752, 480)),
    "euroc-zoom": (EUROC, [2000.0, 2000.0, 376.0, 240.0], (130, 70)),     # taps shared by many pixels: tiny boxes
    "euroc-shrink": (EUROC, [60.0, 60.0, 100.0, 60.0], (200, 120)),       # 7.6 source pixels per step: boxes over the budget
    "hd-inner": (HD, [356.017 * 1920 / 752, 418.236 * 1080 / 480, 362.992 * 1920 / 752, 250.272 * 1080 / 480], (1920, 1080)),
}


def _same(got, want):
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    nbad = int((got.cpu().numpy() != want).sum())
    assert nbad == 0, f"{nbad} of {want.size} bytes differ"


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("case", list(CASES))
def test_staged_equals_twin(case, dev):
    spec, K_new, out_wh = CASES[case]
    ws, hs = spec["wh"]
    tab = twin.table(spec["model"], spec["K"], spec["dist"], K_new, out_wh)
    boxes = staged.tile_boxes(tab, hs, ws)
    share = staged.staged_share(boxes)
    print(case, "tiles staged:", share)
    if case in ("small-same", "euroc-inner", "hd-inner", "euroc-zoom"):
        assert share > 0.9                      # the LDS path is what runs
    if case == "euroc-shrink":
        assert share == 0.0                     # every box is over the budget
    batch = 1 if case == "hd-inner" else 2      # the second frame starts at another offset modulo 16 where Hs Ws 3 % 16 != 0
    src = np.stack([twin.make_content("noise" if b == 0 else "extreme", hs, ws, seed=len(case) + b) for b in range(batch)])
    for border in (0, 200):
        _same(staged.remap_staged(_dev(src, dev), _dev(tab, dev), _dev(boxes, dev), border), twin.remap(src, tab, border))


def test_boxes_are_not_trusted(dev):
    """Boxes of another table, boxes outside the source, huge and negative ones: the bytes stay those of the twin."""
    spec, K_new, out_wh = CASES["euroc-inner"]
    ws, hs = spec["wh"]
    tab = twin.table(spec["model"], spec["K"], spec["dist"], K_new, out_wh)
    src = np.stack([twin.make_content("noise", hs, ws, seed=3 + b) for b in range(2)])
    want = twin.remap(src, tab)
    good = staged.tile_boxes(tab, hs, ws)
    rng = np.random.default_rng(0)
    wrong = {
        "shifted": np.roll(good, 7, axis=0),
        "shrunk": np.maximum(good - np.array([0, 0, 9, 1], np.int32), 0).astype(np.int32),
        "outside": (good + np.array([ws, hs, 0, 0], np.int32)).astype(np.int32),
        "negative": (good * -1).astype(np.int32),
        "huge": np.tile(np.array([[0, 0, 2 ** 31 - 1, 2 ** 31 - 1]], np.int32), (len(good), 1)),
        "corner": np.tile(np.array([[ws - 40, hs - 8, 40, 8]], np.int32), (len(good), 1)),     # the buffer's last bytes
        "random": rng.integers(-50, 800, good.shape).astype(np.int32),
    }
    for name, boxes in wrong.items():
        got = staged.remap_staged(_dev(src, dev), _dev(tab, dev), _dev(boxes, dev))
        nbad = int((got.cpu().numpy() != want).sum())
        assert nbad == 0, f"{name}: {nbad} bytes differ"


def test_staged_equals_the_library_kernel_and_repeats(dev):
    from mast3r_slam import camera
    spec, K_new, out_wh = CASES["euroc-inner"]
    ws, hs = spec["wh"]
    tab = _dev(twin.table(spec["model"], spec["K"], spec["dist"], K_new, out_wh), dev)
    boxes = _dev(staged.tile_boxes(tab.cpu().numpy(), hs, ws), dev)
    src = _dev(np.stack([twin.make_content("noise", hs, ws, seed=b) for b in range(3)]), dev)
    a, b = staged.remap_staged(src, tab, boxes), staged.remap_staged(src, tab, boxes)
    assert torch.equal(a, b) and torch.equal(a, camera.remap_bilinear(src, tab))
