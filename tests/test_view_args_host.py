"""Host: the argument handling the view passes share (mast3r_slam/_view_args.py) raises what render.py, consistency.py
and fusion.py raised when each carried its own copy, in the same order.  No GPU."""
import math

import numpy as np
import pytest
import torch

from mast3r_slam import _view_args as VA
from mast3r_slam import consistency, fusion, render
from mast3r_slam.frame import Frame


def frame(k, h, w):
    f = Frame(frame_id=k, img=torch.zeros((h, w, 3), dtype=torch.uint8), T_WC=torch.tensor([[0, 0, 0, 0, 0, 0, 1, 1.0]]))
    f.X_canon, f.C, f.N = torch.ones((h * w, 3)), torch.full((h * w, 1), 2.0), 1
    return f


@pytest.mark.parametrize("K,words", [
    ((0.0, 1.0, 0.0, 0.0), "focal lengths must be positive"), ((1.0, -1.0, 0.0, 0.0), "focal lengths must be positive"),
    ((math.inf, 1.0, 0.0, 0.0), "focal lengths must be positive"), ((math.nan, 1.0, 0.0, 0.0), "focal lengths must be positive"),
    ((1.0, 1.0, math.inf, 0.0), "principal point finite"), ((1.0, 1.0, 0.0, math.nan), "principal point finite"),
    ((1.0, 1.0, 0.0), "K must be (fx, fy, cx, cy) or a 3 x 3 matrix"), (np.eye(4), "K must be (fx, fy, cx, cy) or a 3 x 3 matrix")])
def test_pinhole_messages(K, words):
    with pytest.raises(ValueError) as e:
        VA._pinhole(K, (4, 6))
    assert words in str(e.value)


def test_pinhole_values():
    assert VA._pinhole(None, (4, 6)) == render.default_intrinsics((4, 6))
    assert VA._pinhole(np.array([[2.0, 0, 3], [0, 4.0, 5], [0, 0, 1]]), (4, 6)) == (2.0, 4.0, 3.0, 5.0)
    assert VA._pinhole(torch.tensor([2.0, 4.0, 3.0, 5.0]), (4, 6)) == (2.0, 4.0, 3.0, 5.0)


@pytest.mark.parametrize("kw,words", [
    (dict(size=(0, 4)), "size must be (H, W) with positive entries"), (dict(size=(4,)), "size must be (H, W) with positive entries"),
    (dict(near=-1.0), "need 0 <= near < far"), (dict(near=2.0, far=2.0), "need 0 <= near < far"),
    (dict(near=math.nan), "need 0 <= near < far"), (dict(background=(0, 0, 256)), "background must be three values in 0 ... 255"),
    (dict(background=(0, 0)), "background must be three values in 0 ... 255")])
def test_view_args_messages(kw, words):
    args = dict(size=(4, 6), K=None, near=0.5, far=math.inf, background=(0, 0, 0))
    args.update(kw)
    with pytest.raises(ValueError) as e:
        VA._view_args(**args)
    assert words in str(e.value)
    assert VA._view_args((4, 6), None, 0.5, 9, (1, 2, 3)) == (4, 6, render.default_intrinsics((4, 6)), 0.5, 9.0, (1, 2, 3))


def test_view_pose_and_outputs_messages():
    with pytest.raises(RuntimeError, match="T_WC: must live on the ROCm device"):
        VA._view_pose(torch.zeros(8))                                       # a CPU tensor: the first thing looked at
    with pytest.raises(ValueError, match="out must hold rgb and depth"):
        VA._outputs((torch.zeros(1),), False, 2, 2, "cpu")
    with pytest.raises(ValueError, match="out must hold rgb, depth and index"):
        VA._outputs((torch.zeros(1),) * 2, True, 2, 2, "cpu")


def test_map_camera_order_of_errors():
    """Keyframes of different sizes, then a bad K string, then CPU tensors."""
    mixed, same = [frame(0, 2, 3), frame(1, 3, 2)], [frame(0, 2, 3), frame(1, 2, 3)]
    with pytest.raises(ValueError) as e:
        VA.map_camera(mixed, mixed, "guess", 1.5)
    assert "'estimate'" not in str(e.value)                               # the sizes, not the K word
    with pytest.raises(ValueError, match="or 'estimate', got 'guess'"):
        VA.map_camera(same, same, "guess", 1.5)
    with pytest.raises(ValueError, match="focal lengths must be positive"):
        VA.map_camera(same, same, (0.0, 1.0, 0.0, 0.0), 1.5)
    with pytest.raises(RuntimeError):
        VA.map_camera(same, same, (1.0, 1.0, 0.0, 0.0), 1.5)
    with pytest.raises(RuntimeError):
        VA.map_camera(same, same, "estimate", 1.5)
    empty = VA.map_camera([], [], "estimate", 1.5)
    assert empty == (None, (1, 1), (1.0, 1.0, 0.0, 0.0), None)
    with pytest.raises(ValueError, match="or 'estimate', got 'guess'"):
        VA.map_camera([], [], "guess", 1.5)


def test_the_passes_keep_their_own_order():
    mixed = [frame(0, 2, 3), frame(1, 3, 2)]
    with pytest.raises(ValueError) as e:                                  # multiview_support: the grid before the K word
        consistency.multiview_support(mixed, "guess")
    assert "'estimate'" not in str(e.value)
    with pytest.raises(ValueError, match="or 'estimate', got 'guess'"):    # fuse_tsdf: the K word before the grid
        fusion.fuse_tsdf(mixed, "guess", 0.25, bounds=((0, 0, 0), (1, 1, 1)))
    assert [t.shape for t in consistency.multiview_support([], "guess")] == [(0, 0)] * 3   # an empty map: K is not looked at


def test_workspace_bytes_share_one_body():
    for mod, sym in ((consistency, "m3_consistency_ws_bytes"), (fusion, "m3_tsdf_integrate_ws_bytes")):
        assert mod.workspace_bytes(3, 2145) == VA.planes_workspace_bytes(sym, 3, 2145) == 3 * 64 + 3 * 2145 * 4
        assert mod.workspace_bytes(0, 5) == 0
        with pytest.raises(ValueError, match="unsupported map of 2 x 0 points"):
            mod.workspace_bytes(2, 0)
