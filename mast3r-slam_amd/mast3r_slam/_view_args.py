"""Argument handling shared by the view passes (render, consistency, fusion): the pinhole, a renderer's view, outputs and
pose, the keyframe map with the camera of its own grid, the size of the observation planes.  Values and shapes raise
ValueError before the first device check; a CPU tensor raises RuntimeError."""
from __future__ import annotations

import math
import numpy as np
import torch

from . import _ffi
from .export import _MapTables, _grid_size, _map_tables, _with_pointmap


def _pinhole(K, size):
    if K is None:
        from .render import default_intrinsics                              # render imports this module
        return default_intrinsics(size)
    if isinstance(K, torch.Tensor):
        K = K.detach().cpu().tolist()
    K = np.asarray(K, dtype=np.float64)
    if K.shape == (3, 3):
        K = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    if K.shape != (4,):
        raise ValueError(f"K must be (fx, fy, cx, cy) or a 3 x 3 matrix, got shape {K.shape}")
    fx, fy, cx, cy = (float(v) for v in K)
    if not (0.0 < fx < math.inf and 0.0 < fy < math.inf and math.isfinite(cx) and math.isfinite(cy)):
        raise ValueError(f"focal lengths must be positive and the principal point finite, got {(fx, fy, cx, cy)}")
    return fx, fy, cx, cy


def _view_args(size, K, near, far, background):
    """(H, W, (fx, fy, cx, cy), near, far, background) of a view, checked: ValueError for anything a renderer rejects."""
    if len(size) != 2 or int(size[0]) <= 0 or int(size[1]) <= 0:
        raise ValueError(f"size must be (H, W) with positive entries, got {size}")
    hv, wv = int(size[0]), int(size[1])
    pinhole = _pinhole(K, (hv, wv))
    near, far = float(near), float(far)
    if not (0.0 <= near < far):
        raise ValueError(f"need 0 <= near < far, got near={near}, far={far}")
    bg = tuple(int(v) for v in background)
    if len(bg) != 3 or any(v < 0 or v > 255 for v in bg):
        raise ValueError(f"background must be three values in 0 ... 255, got {background}")
    return hv, wv, pinhole, near, far, bg


def _outputs(out, return_index: bool, hv: int, wv: int, dev):
    """`out` checked, or freshly allocated: (rgb, depth[, index])."""
    if out is None:
        out = (torch.empty((hv, wv, 3), dtype=torch.uint8, device=dev), torch.empty((hv, wv), dtype=torch.float32, device=dev))
        if return_index:
            out += (torch.empty((hv, wv), dtype=torch.int64, device=dev),)
    if len(out) != (3 if return_index else 2):
        raise ValueError(f"out must hold {'rgb, depth and index' if return_index else 'rgb and depth'}")
    shapes = ((hv, wv, 3), (hv, wv), (hv, wv))
    for t, dt, name, shape in zip(out, (torch.uint8, torch.float32, torch.int64), ("rgb", "depth", "index"), shapes):
        if _ffi.check(t, dt, f"out {name}", shape).data_ptr() != t.data_ptr():
            raise ValueError(f"out {name} must be contiguous")
    return tuple(out)


def _view_pose(T_WC) -> torch.Tensor:
    view = _ffi.check(T_WC, torch.float32, "T_WC").reshape(-1)
    if view.numel() != 8:
        raise ValueError(f"T_WC must have 8 elements (t, q xyzw, s), got {tuple(T_WC.shape)}")
    return view


def _map_frames(keyframes) -> list:
    return keyframes.frames if isinstance(keyframes, _MapTables) else _with_pointmap(keyframes)


def _check_K_word(K) -> None:
    if isinstance(K, str) and K != "estimate":
        raise ValueError(f"K must be a 3 x 3 matrix, (fx, fy, cx, cy) or 'estimate', got {K!r}")


def map_camera(keyframes, frames, K, c_conf_threshold):
    """(tables, (H, W), (fx, fy, cx, cy), poses) of `keyframes` and K as multiview_support and fuse_tsdf take them, with
    frames = _map_frames(keyframes), which the caller has; K "estimate" is intrinsics.estimate_intrinsics under
    c_conf_threshold.  poses: float32 [K,8] gathered from the frames' T_WC on the device, so a captured call follows
    poses updated in place.  Raises, in this order, for keyframes of different sizes (or N != H * W), a bad K word, CPU
    tensors.  An empty map: no tables, no poses, the grid (1, 1)."""
    if not frames:
        _check_K_word(K)
        return None, (1, 1), (1.0, 1.0, 0.0, 0.0) if isinstance(K, str) else _pinhole(K, (1, 1)), None
    h, w = _grid_size(frames)
    _check_K_word(K)
    if not isinstance(K, str):
        K = _pinhole(K, (h, w))
    m = keyframes if isinstance(keyframes, _MapTables) else _map_tables(frames)   # RuntimeError: CPU tensors
    if isinstance(K, str):
        from .intrinsics import estimate_intrinsics
        K = _pinhole(estimate_intrinsics(m, c_conf_threshold=c_conf_threshold).K, (h, w))
    poses = torch.cat([_ffi.check(f.T_WC.reshape(1, 8), torch.float32, "T_WC") for f in m.frames])
    return m, (h, w), K, poses


def planes_workspace_bytes(symbol: str, k: int, n: int) -> int:
    """Bytes of the inverse-pose table and the observation planes of k keyframes of n pixels, by the C function `symbol`."""
    b = int(getattr(_ffi.lib(), symbol)(int(k), int(n)))
    if b <= 0 and k:
        raise ValueError(f"unsupported map of {k} x {n} points (limit 2^31 - 1 points)")
    return b
