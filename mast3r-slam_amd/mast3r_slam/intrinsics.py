"""Camera intrinsics from the keyframes' own pointmaps, estimated on the device (csrc/intrinsics.hip).

The uncalibrated pipeline gets a pointmap per keyframe in that keyframe's camera frame and never a camera.  The
DUSt3R / MASt3R family recovers the focal length from the pointmap itself: with pixel offsets (u, v) from the principal
point and camera points (x, y, z),

    f  =  argmin  sum |(u, v) - f (x / z, y / z)|          (plain norms: robust against wrong points)

found by Weiszfeld re-weighting from the least-squares start f_0 = sum pq / sum qq, pq = a u + b v, qq = a a + b b,
a = x / z, b = y / z.  A pixel takes part when it passes export.collect_map's confidence rule (C / N_k >
c_conf_threshold, None: no test), its point is finite and z > z_min.  Integer pixel coordinates are pixel centres, as
in the renderer.

estimate_focal runs `iters` steps for every keyframe in iters + 3 launches, whatever the number of keyframes, reads
nothing back and allocates nothing when `out` and `workspace` are given, so it can be captured into a graph; two calls
give identical bytes.  estimate_intrinsics makes the one host read and reduces the keyframes to one pinhole.  CPU
tensors raise RuntimeError: there is no CPU path.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _ffi
from ._mesh_args import take_workspace
from .export import _MapTables, _conf_gate, _map_tables, _with_pointmap
from .render import _frame_size

__all__ = ["estimate_focal", "estimate_intrinsics", "intrinsics_from_rows", "IntrinsicsEstimate"]

MAX_ITERS = 64                                                         # include/m3slam.h


@dataclass
class IntrinsicsEstimate:
    """One pinhole for the map.  K: 3 x 3 float64 with fx = fy = focal; principal_point (cx, cy) and size (H, W) as
    given to the estimate; per keyframe the Weiszfeld focal, the least-squares focal, the number of pixels that took
    part and the mean residual in pixels."""
    K: np.ndarray
    focal: float
    principal_point: tuple
    size: tuple
    focal_per_keyframe: np.ndarray
    focal_lsq: np.ndarray
    count: np.ndarray
    residual_px: np.ndarray


def workspace_bytes(k: int, n: int) -> int:
    """Bytes of the partial-sum buffer estimate_focal needs for k keyframes of n pixels."""
    b = int(_ffi.lib().m3_focal_ws_bytes(int(k), int(n)))
    if b <= 0:
        raise ValueError(f"unsupported map of {k} x {n} points (limit 2^31 - 1 points)")
    return b


def _geometry(keyframes, size, principal_point):
    """(n or None for an empty map, (H, W) or None, (cx, cy) or None) with the defaults filled in; ValueError when they
    do not fit the keyframes.  Looks at shapes only: nothing is copied or queued."""
    if isinstance(keyframes, _MapTables):
        frames, n = keyframes.frames, keyframes.n
    else:
        frames = _with_pointmap(keyframes)
        n = frames[0].X_canon.reshape(-1, 3).shape[0] if frames else None
    if size is None and frames:
        size = _frame_size(frames[0].img)
    if size is not None:
        if len(size) != 2 or int(size[0]) <= 0 or int(size[1]) <= 0:
            raise ValueError(f"size must be (H, W) with positive entries, got {size}")
        size = (int(size[0]), int(size[1]))
        if n is not None and size[0] * size[1] != n:
            raise ValueError(f"size {size} has {size[0] * size[1]} pixels, the keyframes' pointmaps have {n} points")
    if principal_point is None:
        pp = None if size is None else ((size[1] - 1) / 2.0, (size[0] - 1) / 2.0)
    else:
        if len(principal_point) != 2:
            raise ValueError(f"principal_point must be (cx, cy), got {principal_point}")
        pp = (float(principal_point[0]), float(principal_point[1]))
        if not (math.isfinite(pp[0]) and math.isfinite(pp[1])):
            raise ValueError(f"principal_point must be finite, got {principal_point}")
    return n, size, pp


def _scalars(z_min, iters):
    if isinstance(iters, bool) or int(iters) != iters or not 0 <= int(iters) <= MAX_ITERS:
        raise ValueError(f"iters must be an integer in 0 ... {MAX_ITERS}, got {iters}")
    z_min = float(z_min)
    if not z_min >= 0.0:
        raise ValueError(f"z_min must be >= 0, got {z_min}")
    return z_min, int(iters)


def estimate_focal(keyframes, size: Optional[Sequence[int]] = None, principal_point: Optional[Sequence[float]] = None,
                   c_conf_threshold: Optional[float] = 1.5, z_min: float = 0.0, iters: int = 10, out=None,
                   workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Device float64 [K,4] with one row per keyframe: the focal after `iters` Weiszfeld steps, the least-squares focal
    f_0, the number of pixels that took part and the mean residual |(u, v) - f (x / z, y / z)| in pixels.  A keyframe
    without a valid pixel gives (NaN, NaN, 0, NaN); nothing is clamped.

    `keyframes` as collect_map / render_map take them, or the result of render.map_tables (then no host copy is made
    and the call can be captured).  size = (H, W), default the keyframes' own image size; principal_point = (cx, cy),
    default ((W - 1) / 2, (H - 1) / 2); c_conf_threshold None: no confidence test; a pixel needs z > z_min.  `out`: a
    contiguous float64 [K,4] device tensor to write into; `workspace`: a uint8 device tensor of workspace_bytes(K, N).
    An empty map gives a [0,4] tensor and no launch."""
    z_min, iters = _scalars(z_min, iters)
    n, size, pp = _geometry(keyframes, size, principal_point)
    m = keyframes if isinstance(keyframes, _MapTables) else _map_tables(keyframes)
    if m is None:
        return torch.empty((0, 4), dtype=torch.float64, device="cuda" if torch.cuda.is_available() else "cpu")
    dev = m.device
    ws_bytes = workspace_bytes(m.k, m.n)
    if out is None:
        out = torch.empty((m.k, 4), dtype=torch.float64, device=dev)
    if _ffi.check(out, torch.float64, "out", (m.k, 4)).data_ptr() != out.data_ptr():
        raise ValueError("out must be contiguous")
    workspace = take_workspace(workspace, ws_bytes, dev, owner=None)
    use, thr = _conf_gate(c_conf_threshold)
    _ffi.call("m3_focal_estimate", _ffi.ptr(m.table[0]), _ffi.ptr(m.table[1]), _ffi.ptr(m.nk), m.k, m.n, size[0], size[1],
              use, thr, pp[0], pp[1], z_min, iters, _ffi.ptr(workspace), ws_bytes, _ffi.ptr(out), _ffi.stream_ptr())
    return out


def intrinsics_from_rows(rows, size: Sequence[int], principal_point: Sequence[float],
                         min_pixels: int = 1024) -> IntrinsicsEstimate:
    """The map's pinhole from the [K,4] rows of estimate_focal (host array): focal = numpy.median of the per-keyframe
    focals over the keyframes with count >= min_pixels and a finite focal.  ValueError when none qualifies: no default
    is substituted."""
    r = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    count = r[:, 2].astype(np.int64)
    good = (count >= int(min_pixels)) & np.isfinite(r[:, 0])
    if not good.any():
        raise ValueError(f"no keyframe has a finite focal estimate from at least {int(min_pixels)} pixels "
                         f"(valid pixels per keyframe: {count.tolist()})")
    focal = float(np.median(r[good, 0]))
    cx, cy = float(principal_point[0]), float(principal_point[1])
    K = np.array([[focal, 0.0, cx], [0.0, focal, cy], [0.0, 0.0, 1.0]], dtype=np.float64)
    return IntrinsicsEstimate(K=K, focal=focal, principal_point=(cx, cy), size=(int(size[0]), int(size[1])),
                              focal_per_keyframe=r[:, 0].copy(), focal_lsq=r[:, 1].copy(), count=count,
                              residual_px=r[:, 3].copy())


def estimate_intrinsics(keyframes, size: Optional[Sequence[int]] = None,
                        principal_point: Optional[Sequence[float]] = None, c_conf_threshold: Optional[float] = 1.5,
                        z_min: float = 0.0, iters: int = 10, min_pixels: int = 1024) -> IntrinsicsEstimate:
    """estimate_focal, read back once, reduced to one IntrinsicsEstimate (see intrinsics_from_rows)."""
    _scalars(z_min, iters)
    n, hw, pp = _geometry(keyframes, size, principal_point)
    if n is None:
        raise ValueError("no keyframe has a pointmap (valid pixels per keyframe: [])")
    rows = estimate_focal(keyframes, hw, pp, c_conf_threshold, z_min, iters)
    return intrinsics_from_rows(rows.cpu().numpy(), hw, pp, min_pixels)
