"""Fixed-radius neighbourhoods of the exported point cloud on the device, and the two passes on top of them: normals
and the radius outlier filter (csrc/cloud.hip).

A cloud without normals cannot go into a Poisson reconstruction or a surfel viewer, and after the confidence and
consistency gates isolated floaters remain.  Both need the same thing: for every point, the points within a radius.
cloud_neighbors answers that on a uniform grid over an open-addressing table; cloud_normals and remove_radius_outliers
are built on it, and are applied to what collect_map / SLAM.reconstruction return:

    pts = slam.reconstruction(voxel_size=v, return_index=True)
    n = cloud_normals(pts, radius=3*v, toward=source_viewpoints(slam.keyframes, pts[2]))
    save_ply_normals(path, pts[0], pts[1], n)

    neighbours of i    every finite j, i included, with (dx dx + dy dy) + dz dz <= r r in float64; inclusive
    count, moments     |N(i)| and nine integer sums of the offsets quantised to r / 2^20: first and second moments
    normal             the unit eigenvector of the smallest eigenvalue of the covariance of the offsets; (0,0,0) below
                       min_points neighbours or without spread; turned towards `toward` (the camera that saw the point)
    variation          l0 / (l0 + l1 + l2): 0 on a plane, 1/3 for an isotropic blob
    radius filter      a point stays when at least min_neighbors OTHER points lie within the radius

The exact rule is in include/m3slam.h.  Counts and moments are integer sums over a set: two calls give identical bytes,
and so do two orders of the input rows.  The filter's threshold counts other points - the project's own rule, close to
but not claimed to be Open3D's remove_radius_outlier, whose nb_points includes the query.  k-nearest-neighbour queries,
the statistical (mean k-NN distance) outlier filter, normal propagation over a minimum spanning tree for clouds without
viewpoints, per-point radii, a `normals=` argument on the driver methods and normals in render_map are left out.  CPU
tensors raise RuntimeError: there is no CPU path.
"""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from . import _ffi
from .export import _check_workspace, _with_pointmap

__all__ = ["cloud_neighbors", "cloud_normals", "source_viewpoints", "remove_radius_outliers", "CloudNeighbors",
           "workspace_bytes"]

CloudNeighbors = namedtuple("CloudNeighbors", ["count", "moments", "out_of_range"])
CloudNeighbors.__doc__ = ("count int32 [M]: the points within the radius, the point itself included, 0 for a point that is "
                          "not finite; moments int64 [M,9] (sum qx qy qz, qx qx, qx qy, qx qz, qy qy, qy qz, qz qz of the "
                          "offsets times 2^20 / r, rounded) or None; out_of_range: always 0 - the call raises otherwise - "
                          "or None under stream capture, where nothing is read back.")

MAX_POINTS = 2 ** 30                                                    # include/m3slam.h
_HDR_WORDS = 4                                                          # out of range, points in cells, kept rows, 0


def workspace_bytes(M: int) -> int:
    """Bytes of the workspace the calls of this module need for a cloud of M points."""
    b = int(_ffi.lib().m3_cloud_ws_bytes(int(M)))
    if b <= 0:
        raise ValueError(f"unsupported cloud of {M} points (0 ... 2^30)")
    return b


def _radius(radius) -> tuple:
    """(r as fp32, scale = 2^20 / r in float64): ValueError before any device call."""
    if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)):
        raise ValueError(f"radius must be a number, got {radius!r}")
    with np.errstate(over="ignore"):
        r = float(np.float32(radius))
    if not math.isfinite(r) or not r > 0.0:
        raise ValueError(f"radius must be positive and finite (as fp32), got {radius}")
    return r, 2.0 ** 20 / r


def _points(points, name: str = "points") -> None:
    if not isinstance(points, torch.Tensor) or points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
        got = f"{points.dtype} {tuple(points.shape)}" if isinstance(points, torch.Tensor) else type(points).__name__
        raise ValueError(f"{name} must be a {torch.float32} [n,3] tensor, got {got}")
    if points.shape[0] > MAX_POINTS:
        raise ValueError(f"{points.shape[0]} points, the limit is 2^30")


def _workspace(workspace: Optional[torch.Tensor], m: int, dev) -> torch.Tensor:
    ws_bytes = workspace_bytes(m)
    if workspace is None:
        workspace = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    _check_workspace(workspace, ws_bytes)
    if workspace.device != dev:
        raise ValueError(f"the cloud lives on {dev}, the workspace on {workspace.device}")
    return workspace


def _too_small(radius: float, n: int) -> ValueError:
    return ValueError(f"radius too small for the extent of the cloud: at radius {radius}, {n} points have a cell "
                      "coordinate beyond +-2^20")


def _neighbors(points: torch.Tensor, r: float, scale: float, moments: bool, ws: torch.Tensor):
    """Queue the seven launches: (count, moments or None)."""
    m, dev = int(points.shape[0]), points.device
    count = torch.empty((m,), dtype=torch.int32, device=dev)
    mom = torch.empty((m, 9), dtype=torch.int64, device=dev) if moments else None
    _ffi.call("m3_cloud_neighbors", _ffi.ptr(points), m, r, scale, _ffi.ptr(count), _ffi.ptr(mom), _ffi.ptr(ws), ws.numel(),
              _ffi.stream_ptr())
    return count, mom


def _header(ws: torch.Tensor, r: float):
    """The header words, or None under stream capture; ValueError when a point is out of range.  The one synchronisation."""
    if torch.cuda.is_current_stream_capturing():
        return None
    hdr = ws[:4 * _HDR_WORDS].view(torch.int32).tolist()
    if hdr[0]:
        raise _too_small(r, hdr[0])
    return hdr


def cloud_neighbors(points, radius, moments: bool = True, workspace: Optional[torch.Tensor] = None) -> CloudNeighbors:
    """CloudNeighbors(count, moments, out_of_range) of the points float32 [M,3] (a device tensor) at `radius`.

    count int32 [M] is the number of points within the radius of each point, itself included (duplicates count; a point
    that is not finite has 0 and is counted nowhere); moments int64 [M,9] holds the first and second moments of their
    offsets in units of radius / 2^20, None with moments=False.  The call queues 7 launches and reads one 16-byte header
    back: its only synchronisation.  ValueError ("radius too small for the extent of the cloud") when a point's grid
    cell reaches +-2^20.  workspace: a 16-byte aligned uint8 device tensor of workspace_bytes(M); with it the call can
    be captured into a graph - nothing is read back then, out_of_range is None, and the first int32 of the workspace
    holds the number after a replay.  RuntimeError for a CPU tensor."""
    r, scale = _radius(radius)
    _points(points)
    points = _ffi.check(points, torch.float32, "points")
    m, dev = int(points.shape[0]), points.device
    if m == 0:
        return CloudNeighbors(torch.empty((0,), dtype=torch.int32, device=dev),
                              torch.empty((0, 9), dtype=torch.int64, device=dev) if moments else None, 0)
    ws = _workspace(workspace, m, dev)
    count, mom = _neighbors(points, r, scale, bool(moments), ws)
    hdr = _header(ws, r)
    return CloudNeighbors(count, mom, None if hdr is None else hdr[0])


def cloud_normals(points, radius, toward: Optional[torch.Tensor] = None, min_points: int = 3, return_variation: bool = False,
                  workspace: Optional[torch.Tensor] = None):
    """Normals float32 [M,3] of the points float32 [M,3] - or of the whole tuple collect_map / SLAM.reconstruction
    return - from the points within `radius` of each; with return_variation also the surface variation float32 [M].

    The normal is the direction of least spread of the neighbourhood, unit length; a point with fewer than min_points
    points in its neighbourhood (itself included), one whose neighbourhood has no spread and one that is not finite
    get (0,0,0) and variation 0.  toward: a [3] or [M,3] float32 device tensor - one viewpoint, or one per point, as
    source_viewpoints gives them; each normal is turned to face its viewpoint.  Without it the component of largest
    magnitude is made positive.  radius = 3 voxel edges of a thinned cloud gives about 28 neighbours on a surface.

    8 launches and the one 16-byte read of cloud_neighbors; ValueError as there, and for min_points < 1 or a `toward`
    of another shape, dtype or device.  workspace as in cloud_neighbors.  Identical bytes on every call."""
    if isinstance(points, (tuple, list)):
        if len(points) < 2:
            raise ValueError("a cloud is (points, colors[, index]), passed whole, or the points alone")
        points = points[0]
    r, scale = _radius(radius)
    if isinstance(min_points, bool) or not isinstance(min_points, (int, np.integer)) or min_points < 1 or min_points >= 2 ** 31:
        raise ValueError(f"min_points must be an integer >= 1, got {min_points!r}")
    _points(points)
    m = int(points.shape[0])
    stride = 0
    if toward is not None:
        if not isinstance(toward, torch.Tensor) or toward.dtype != torch.float32 or tuple(toward.shape) not in ((3,), (m, 3)):
            got = f"{toward.dtype} {tuple(toward.shape)}" if isinstance(toward, torch.Tensor) else type(toward).__name__
            raise ValueError(f"toward must be a {torch.float32} [3] or [{m},3] tensor, got {got}")
        stride = 3 if toward.dim() == 2 else 0
    points = _ffi.check(points, torch.float32, "points")
    dev = points.device
    if toward is not None:
        toward = _ffi.check(toward, torch.float32, "toward")
        if toward.device != dev:
            raise ValueError(f"the cloud lives on {dev}, toward on {toward.device}")
    normals = torch.empty((m, 3), dtype=torch.float32, device=dev)
    variation = torch.empty((m,), dtype=torch.float32, device=dev) if return_variation else None
    if m:
        ws = _workspace(workspace, m, dev)
        count, mom = _neighbors(points, r, scale, True, ws)
        _ffi.call("m3_cloud_normals", _ffi.ptr(points), m, _ffi.ptr(count), _ffi.ptr(mom), _ffi.ptr(toward), stride,
                  int(min_points), _ffi.ptr(normals), _ffi.ptr(variation), _ffi.stream_ptr())
        _header(ws, r)
    return (normals, variation) if return_variation else normals


def source_viewpoints(keyframes, index: torch.Tensor) -> torch.Tensor:
    """float32 [M,3]: for every source index of collect_map(..., return_index=True) - k * N + n over the keyframes that
    have a pointmap - the camera centre of keyframe k, the translation of its T_WC.  The `toward` of cloud_normals."""
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int64 or index.dim() != 1:
        got = f"{index.dtype} {tuple(index.shape)}" if isinstance(index, torch.Tensor) else type(index).__name__
        raise ValueError(f"index must be a {torch.int64} [M] tensor, got {got}")
    frames = _with_pointmap(keyframes)
    if not frames:
        if index.numel():
            raise ValueError("no keyframe has a pointmap")
        return torch.empty((0, 3), dtype=torch.float32, device=index.device)
    n = frames[0].X_canon.reshape(-1, 3).shape[0]
    centres = torch.cat([f.T_WC.reshape(1, 8)[:, :3] for f in frames]).to(device=index.device, dtype=torch.float32)
    k = torch.div(index, n, rounding_mode="floor")
    if index.numel() and (int(k.min()) < 0 or int(k.max()) >= len(frames)):
        raise ValueError(f"index names keyframes {int(k.min())} ... {int(k.max())}, the map has {len(frames)}")
    return centres[k]


def remove_radius_outliers(points, colors=None, index=None, radius=None, min_neighbors=None, return_rows: bool = False):
    """The cloud without the points that have fewer than `min_neighbors` OTHER points within `radius`: (points, colors)
    or (points, colors, index) as passed - whole, as collect_map / SLAM.reconstruction return it, or unpacked - in input
    order, with the index gathered; return_rows adds the kept input rows, int64.

    Points that are not finite are always dropped; exact duplicates are neighbours of each other.  min_neighbors counts
    other points: the project's own rule (Open3D's nb_points includes the query).  The neighbour pass with counts only
    (7 launches), 2 for the kept count, one 16-byte read, one scatter.  ValueError without radius or min_neighbors, for
    min_neighbors < 0, mismatched rows, and ("radius too small for the extent of the cloud") when a point's grid cell
    reaches +-2^20; RuntimeError for CPU tensors."""
    if isinstance(points, (tuple, list)):
        if len(points) not in (2, 3) or colors is not None or index is not None:
            raise ValueError("a cloud is (points, colors[, index]), passed whole or unpacked")
        points, colors, index = (tuple(points) + (None,))[:3]
    if radius is None or min_neighbors is None:
        raise ValueError("radius and min_neighbors are required")
    r, scale = _radius(radius)
    if isinstance(min_neighbors, bool) or not isinstance(min_neighbors, (int, np.integer)) or not 0 <= min_neighbors < 2 ** 31 - 1:
        raise ValueError(f"min_neighbors must be an integer >= 0, got {min_neighbors!r}")
    _points(points)
    m = int(points.shape[0])
    if not isinstance(colors, torch.Tensor) or colors.dtype != torch.uint8 or tuple(colors.shape) != (m, 3):
        got = f"{colors.dtype} {tuple(colors.shape)}" if isinstance(colors, torch.Tensor) else type(colors).__name__
        raise ValueError(f"colors must be a {torch.uint8} [{m},3] tensor, got {got}")
    if index is not None and (not isinstance(index, torch.Tensor) or index.dtype != torch.int64 or tuple(index.shape) != (m,)):
        got = f"{index.dtype} {tuple(index.shape)}" if isinstance(index, torch.Tensor) else type(index).__name__
        raise ValueError(f"index must be a {torch.int64} [{m}] tensor, got {got}")
    points = _ffi.check(points, torch.float32, "points")
    colors = _ffi.check(colors, torch.uint8, "colors")
    dev = points.device
    if index is not None:
        index = _ffi.check(index, torch.int64, "index")
    if colors.device != dev or (index is not None and index.device != dev):
        raise ValueError(f"points live on {dev}, colors on {colors.device}" + (f", index on {index.device}" if index is not None else ""))
    m2 = 0
    if m:
        ws = _workspace(None, m, dev)
        count, _ = _neighbors(points, r, scale, False, ws)
        _ffi.call("m3_cloud_radius_count", _ffi.ptr(count), m, int(min_neighbors), _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr())
        m2 = _header(ws, r)[2]                                          # the one synchronisation
    p2 = torch.empty((m2, 3), dtype=torch.float32, device=dev)
    c2 = torch.empty((m2, 3), dtype=torch.uint8, device=dev)
    i2 = torch.empty((m2,), dtype=torch.int64, device=dev) if index is not None else None
    rows = torch.empty((m2,), dtype=torch.int64, device=dev) if return_rows else None
    if m2:
        _ffi.call("m3_cloud_radius_scatter", _ffi.ptr(points), _ffi.ptr(colors), _ffi.ptr(index), _ffi.ptr(count), m,
                  int(min_neighbors), _ffi.ptr(ws), ws.numel(), m2, _ffi.ptr(p2), _ffi.ptr(c2), _ffi.ptr(i2), _ffi.ptr(rows),
                  _ffi.stream_ptr())
    out = (p2, c2) if index is None else (p2, c2, i2)
    return out + (rows,) if return_rows else out
