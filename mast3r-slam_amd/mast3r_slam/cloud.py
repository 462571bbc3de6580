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
but not claimed to be Open3D's remove_radius_outlier, whose nb_points includes the query.

On the same index: cloud_knn, the k nearest points within a radius of every point or of another
set of queries; remove_statistical_outliers, which drops the points whose mean distance to their k nearest is more than
std_ratio deviations above the cloud's mean - a threshold that adapts to the cloud, where the radius filter has one
absolute one; and cloud_normals_knn, normals over the k nearest instead of everything within the radius.

    order              by key = (bits(d2) & ~(2^30 - 1)) | row, ascending: squared distance to 22 mantissa bits, ties to
                       the lower row - two candidates whose d2 differ only in the dropped bits are ordered by row
    q                  the sum over a complete row's k neighbours of floor(sqrt(rint(d2 2^32 / r^2))), an integer

Unbounded k-NN, normal propagation over a minimum spanning tree for clouds without viewpoints, per-point radii, cross
queries sorted through an index of their own, a `normals=` argument on the driver methods and normals in render_map are
left out.  CPU tensors raise RuntimeError: there is no CPU path.
"""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from . import _ffi
from ._mesh_args import take_workspace
from .export import _with_pointmap

__all__ = ["cloud_neighbors", "cloud_normals", "source_viewpoints", "remove_radius_outliers", "CloudNeighbors",
           "workspace_bytes", "cloud_knn", "KnnResult", "remove_statistical_outliers", "cloud_normals_knn", "MAX_K"]

CloudNeighbors = namedtuple("CloudNeighbors", ["count", "moments", "out_of_range"])
CloudNeighbors.__doc__ = ("count int32 [M]: the points within the radius, the point itself included, 0 for a point that is "
                          "not finite; moments int64 [M,9] (sum qx qy qz, qx qx, qx qy, qx qz, qy qy, qy qz, qz qz of the "
                          "offsets times 2^20 / r, rounded) or None; out_of_range: always 0 - the call raises otherwise - "
                          "or None under stream capture, where nothing is read back.")

KnnResult = namedtuple("KnnResult", ["index", "dist2", "found", "out_of_range"])
KnnResult.__doc__ = ("index int32 [Q,k]: the rows of the nearest points in ascending key order, then -1; dist2 float32 [Q,k]: "
                     "their squared distances (float64, rounded once), then +inf; found int32 [Q] = min(k, the candidates "
                     "within the radius); out_of_range: always 0 - the call raises otherwise - or None under stream capture.")

MAX_POINTS = 2 ** 30                                                    # include/m3slam.h
MAX_K = 64
_KNN_HDR_WORDS = 16                                                     # + queries out of range, n, S1, S2lo, S2hi
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
    return take_workspace(workspace, workspace_bytes(m), dev, owner="the cloud lives")


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


def _normals_args(points, toward, min_points):
    """(points, toward, stride), checked as cloud_normals documents."""
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
    return points, toward, stride


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
    points, toward, stride = _normals_args(points, toward, min_points)
    m, dev = int(points.shape[0]), points.device
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
    points, colors, index = _unpack(points, colors, index)
    if radius is None or min_neighbors is None:
        raise ValueError("radius and min_neighbors are required")
    r, scale = _radius(radius)
    if isinstance(min_neighbors, bool) or not isinstance(min_neighbors, (int, np.integer)) or not 0 <= min_neighbors < 2 ** 31 - 1:
        raise ValueError(f"min_neighbors must be an integer >= 0, got {min_neighbors!r}")
    points, colors, index = _cloud(points, colors, index)
    m, dev = int(points.shape[0]), points.device
    m2 = 0
    ws = count = None
    if m:
        ws = _workspace(None, m, dev)
        count, _ = _neighbors(points, r, scale, False, ws)
        _ffi.call("m3_cloud_radius_count", _ffi.ptr(count), m, int(min_neighbors), _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr())
        m2 = _header(ws, r)[2]                                          # the one synchronisation
    return _scatter("m3_cloud_radius_scatter", points, colors, index, count, int(min_neighbors), ws, m2, return_rows)


def _unpack(points, colors, index):
    if isinstance(points, (tuple, list)):
        if len(points) not in (2, 3) or colors is not None or index is not None:
            raise ValueError("a cloud is (points, colors[, index]), passed whole or unpacked")
        points, colors, index = (tuple(points) + (None,))[:3]
    return points, colors, index


def _cloud(points, colors, index):
    """The three tensors of a cloud, checked: ValueError for what no device call is needed to refuse, then RuntimeError for
    CPU tensors."""
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
    return points, colors, index


def _scatter(entry: str, points, colors, index, values, bound: int, ws, m2: int, return_rows: bool):
    """The ordered compaction of both filters: the m2 rows whose `values` pass the predicate of `entry` at `bound`."""
    m, dev = int(points.shape[0]), points.device
    p2 = torch.empty((m2, 3), dtype=torch.float32, device=dev)
    c2 = torch.empty((m2, 3), dtype=torch.uint8, device=dev)
    i2 = torch.empty((m2,), dtype=torch.int64, device=dev) if index is not None else None
    rows = torch.empty((m2,), dtype=torch.int64, device=dev) if return_rows else None
    if m2:
        _ffi.call(entry, _ffi.ptr(points), _ffi.ptr(colors), _ffi.ptr(index), _ffi.ptr(values), m, bound, _ffi.ptr(ws), ws.numel(),
                  m2, _ffi.ptr(p2), _ffi.ptr(c2), _ffi.ptr(i2), _ffi.ptr(rows), _ffi.stream_ptr())
    out = (p2, c2) if index is None else (p2, c2, i2)
    return out + (rows,) if return_rows else out


# ---- k nearest within the radius -------------------------------------------------------------------------------------
def _k(k) -> int:
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= MAX_K:
        raise ValueError(f"k must be an integer in 1 ... {MAX_K}, got {k!r}")
    return int(k)


def _knn(points: torch.Tensor, r: float, k: int, queries: Optional[torch.Tensor], ws: torch.Tensor):
    """Queue the seven launches: (index, dist2, found)."""
    m, dev = int(points.shape[0]), points.device
    q = m if queries is None else int(queries.shape[0])
    index = torch.empty((q, k), dtype=torch.int32, device=dev)
    dist2 = torch.empty((q, k), dtype=torch.float32, device=dev)
    found = torch.empty((q,), dtype=torch.int32, device=dev)
    _ffi.call("m3_knn_query", _ffi.ptr(points), m, r, _ffi.ptr(queries), q, k, _ffi.ptr(index), _ffi.ptr(dist2), _ffi.ptr(found),
              _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr())
    return index, dist2, found


def _knn_header(ws: torch.Tensor, r: float):
    """The 16 header words, or None under stream capture; ValueError when a point or a query is out of range."""
    if torch.cuda.is_current_stream_capturing():
        return None
    hdr = ws[:4 * _KNN_HDR_WORDS].view(torch.int32).tolist()
    if hdr[0]:
        raise _too_small(r, hdr[0])
    if hdr[3]:
        raise ValueError(f"radius too small for the extent of the queries: at radius {r}, {hdr[3]} queries have a cell "
                         "coordinate beyond +-2^20")
    return hdr


def cloud_knn(points, k, radius, queries: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> KnnResult:
    """KnnResult(index, dist2, found, out_of_range): the k nearest points within `radius` of every point of the float32
    [M,3] device tensor `points` - or, with `queries` float32 [Q,3] on the same device, of every query.

    The search is the k nearest WITHIN the radius (Open3D's hybrid search): a query with fewer than k candidates has
    found < k, index -1 and dist2 +inf in the rest of its row.  Without `queries` row i is not its own neighbour; other
    rows at the same position are, at distance 0.  With `queries` nothing is excluded.  Points and queries that are not
    finite find nothing and are found by nobody.  Candidates are ordered by key = (bits(d2) & ~(2^30 - 1)) | row: by
    squared distance (float64) to 22 mantissa bits, ties to the lower row - so two candidates whose d2 differ only in the
    dropped 30 bits are ordered by row, not by distance.  The result is a function of the point set and the query alone:
    identical bytes on every call.  k: an integer in 1 ... 64.

    7 launches and one 64-byte read.  ValueError for a bad k, radius, points or queries (before any device call), and
    ("radius too small for the extent ...") when the grid cell of a point or a query reaches +-2^20.  workspace: as in
    cloud_neighbors - with it the call can be captured; nothing is read back then and out_of_range is None.  RuntimeError
    for CPU tensors."""
    k = _k(k)
    r, _ = _radius(radius)
    _points(points)
    if queries is not None:
        _points(queries, "queries")
        if queries.device != points.device:
            raise ValueError(f"the cloud lives on {points.device}, the queries on {queries.device}")
    points = _ffi.check(points, torch.float32, "points")
    if queries is not None:
        queries = _ffi.check(queries, torch.float32, "queries")
    ws = _workspace(workspace, int(points.shape[0]), points.device)
    index, dist2, found = _knn(points, r, k, queries, ws)
    hdr = _knn_header(ws, r)
    return KnnResult(index, dist2, found, None if hdr is None else hdr[0] + hdr[3])


def cloud_normals_knn(points, radius, k, toward: Optional[torch.Tensor] = None, min_points: int = 3,
                      return_variation: bool = False, workspace: Optional[torch.Tensor] = None, return_moments: bool = False):
    """cloud_normals over an adaptive neighbourhood: point i and its k nearest others within `radius` (cloud_knn's order)
    instead of every point within the radius.  Arguments, outputs and errors are those of cloud_normals; k is an integer
    in 1 ... 64.  return_moments appends (count int32 [M], moments int64 [M,9]) of those neighbourhoods: count = found + 1.
    Where no point has more than k others within the radius they are cloud_neighbors' bytes, and so are the normals.

    9 launches (7 of the k-NN query, the moments of the k nearest, the normals) and one 64-byte read."""
    if isinstance(points, (tuple, list)):
        if len(points) < 2:
            raise ValueError("a cloud is (points, colors[, index]), passed whole, or the points alone")
        points = points[0]
    k = _k(k)
    r, scale = _radius(radius)
    points, toward, stride = _normals_args(points, toward, min_points)
    m, dev = int(points.shape[0]), points.device
    normals = torch.empty((m, 3), dtype=torch.float32, device=dev)
    variation = torch.empty((m,), dtype=torch.float32, device=dev) if return_variation else None
    count = torch.empty((m,), dtype=torch.int32, device=dev)
    mom = torch.empty((m, 9), dtype=torch.int64, device=dev)
    if m:
        ws = _workspace(workspace, m, dev)
        index, _, found = _knn(points, r, k, None, ws)
        _ffi.call("m3_knn_moments", _ffi.ptr(points), m, r, scale, _ffi.ptr(index), _ffi.ptr(found), k, _ffi.ptr(count),
                  _ffi.ptr(mom), _ffi.stream_ptr())
        _ffi.call("m3_cloud_normals", _ffi.ptr(points), m, _ffi.ptr(count), _ffi.ptr(mom), _ffi.ptr(toward), stride,
                  int(min_points), _ffi.ptr(normals), _ffi.ptr(variation), _ffi.stream_ptr())
        _knn_header(ws, r)
    out = (normals, variation) if return_variation else (normals,)
    out = out + (count, mom) if return_moments else out
    return out if len(out) > 1 else out[0]


def _std_ratio(std_ratio) -> float:
    if isinstance(std_ratio, bool) or not isinstance(std_ratio, (int, float, np.integer, np.floating)) or \
            not math.isfinite(float(std_ratio)):
        raise ValueError(f"std_ratio must be a finite number, got {std_ratio!r}")
    return float(std_ratio)


def statistical_threshold(n: int, s1: int, s2: int, std_ratio: float) -> float:
    """T = mu + std_ratio sqrt(var) in float64 from the exact integers n, S1 = sum q, S2 = sum q^2 (include/m3slam.h)."""
    if n < 1:
        return -1.0
    mu = s1 / n
    var = (n * s2 - s1 * s1) / (n * (n - 1)) if n >= 2 else 0.0
    return mu + std_ratio * math.sqrt(var)


def remove_statistical_outliers(points, colors=None, index=None, k: int = 20, std_ratio: float = 2.0, radius=None,
                                return_rows: bool = False, return_stats: bool = False):
    """The cloud without the points whose mean distance to their k nearest neighbours is more than std_ratio standard
    deviations above the mean of that distance over the cloud: (points, colors) or (points, colors, index) as passed -
    whole or unpacked, as for remove_radius_outliers - in input order; return_rows adds the kept input rows, int64;
    return_stats adds a dict(q int32 [M], n, S1, S2, T) last.

    The neighbours are cloud_knn's: the k nearest OTHER points within `radius` (required: the search is bounded).  The
    selection runs in exact integers.  A row is complete when it has k neighbours; q_i is the sum over them of
    floor(sqrt(rint(d2 2^32 / r^2))), the mean distance in units of r / (k 2^16), -1 for a row that is not complete.
    The device adds up n = the complete rows, S1 = sum q and S2 = sum q^2; mu = S1 / n, var = (n S2 - S1^2) / (n (n - 1))
    (0 for n < 2) and T = mu + std_ratio sqrt(var) are float64 operations on exact Python integers, and a row stays iff
    it is complete and q_i <= T.  Identical bytes on every call.

    Against Open3D's remove_statistical_outlier: (1) the radius bound - a point with fewer than k others within `radius`
    is dropped, and it takes no part in mu and var; (2) distances in the integer units above, not float64.  Where every
    point is complete the selection is Open3D's up to arithmetic; nothing more is claimed.

    11 launches (7 of the k-NN query, q and its sums, 2 for the kept count, one scatter) and two reads: the 64-byte
    header with n, S1, S2, then the kept count.  Not capturable, as remove_radius_outliers is not.  ValueError without a
    radius, for k outside 1 ... 64 or not an integer, a std_ratio that is not finite, mismatched rows, and ("radius too
    small for the extent of the cloud") when a point's grid cell reaches +-2^20; RuntimeError for CPU tensors."""
    points, colors, index = _unpack(points, colors, index)
    if radius is None:
        raise ValueError("radius is required: the k nearest are searched within it")
    k = _k(k)
    ratio = _std_ratio(std_ratio)
    r, _ = _radius(radius)
    points, colors, index = _cloud(points, colors, index)
    m, dev = int(points.shape[0]), points.device
    q = torch.empty((m,), dtype=torch.int32, device=dev)
    n = s1 = s2 = m2 = bound = 0
    ws = None
    if m:
        ws = _workspace(None, m, dev)
        nn, _, found = _knn(points, r, k, None, ws)
        _ffi.call("m3_knn_mean_distance", _ffi.ptr(points), m, 2.0 ** 32 / (r * r), _ffi.ptr(nn), _ffi.ptr(found), k, _ffi.ptr(q),
                  _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr())
        hdr = _knn_header(ws, r)                                        # the first read
        u64 = lambda w: (hdr[w] & 0xffffffff) | ((hdr[w + 1] & 0xffffffff) << 32)
        n, s1, s2 = hdr[4], u64(6), u64(8) + (u64(10) << 32)
    t = statistical_threshold(n, s1, s2, ratio)
    if n and t >= 0.0:
        bound = min(int(math.floor(t)), 2 ** 31 - 1)
        _ffi.call("m3_knn_stat_count", _ffi.ptr(q), m, bound, _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr())
        m2 = ws[8:12].view(torch.int32).item()                          # the second read
    out = _scatter("m3_knn_stat_scatter", points, colors, index, q, bound, ws, m2, return_rows)
    return out + (dict(q=q, n=n, S1=s1, S2=s2, T=t),) if return_stats else out
