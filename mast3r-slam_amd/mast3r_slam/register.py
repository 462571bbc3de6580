"""Registration of one point cloud onto another on the device: point-to-point and point-to-plane ICP over Sim(3)
(csrc/icp.hip).

A MASt3R-SLAM map has no metric scale and an arbitrary frame.  register_clouds puts a run onto a reference scan, a
second session onto the first or an exported sub-map back onto the full map, on the uniform-grid index the other cloud
passes use, and stays byte-reproducible as they are:

    pts = slam.reconstruction(voxel_size=v)
    n = cloud_normals(ref, 3*v, ...)
    reg = register_clouds(pts[0], ref, radius=5*v, target_normals=n, with_scale=True)
    moved = reg.apply(pts[0])

    pose               x' = s R x + t in float64 on the device; T = [[s R, t], [0, 1]]
    correspondence     the nearest target point within `radius` of the moved source point rounded to float32: cloud_knn's
                       k = 1 result for that query (same cells, same membership test, same key, ties to the lower row)
    point to point     minimises sum |x' - q|^2 over (translation, rotation[, scale])
    point to plane     minimises sum (n . (x' - q))^2; target rows whose normal is (0,0,0) or not finite are skipped
    step               Gauss-Newton: 36 sums reduced in a fixed tree, LDL^T, Cayley's map for the rotation; no sqrt, sin or
                       cos in an iteration, so the whole trajectory equals the numpy twin's byte for byte
    stop               |translation step| <= tol * radius, |rotation step| <= tol, |scale step| <= tol; or too few pairs /
                       a singular system (status), after which the remaining launches do nothing

The exact rule is in include/m3slam.h.  iterations=30, tol=1e-6 and min_pairs=16 are this project's choices, untuned on
real data.  The iteration never comes back to the host: 6 + 2 * iterations + 2 launches whatever happens, one read of
the state and the history at the end.  Robust kernels and trimming, a normal-compatibility gate, source rows sorted
through the target's cells, multi-scale radii, colour terms, global registration (FPFH, RANSAC) and a driver method are
left out.  CPU tensors raise RuntimeError: there is no CPU path.
"""
from __future__ import annotations

import ctypes
import math
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from . import _ffi
from ._mesh_args import take_workspace
from .cloud import _points, _radius

__all__ = ["register_clouds", "icp_sums", "Registration", "IcpSums", "registration_workspace_bytes", "read_registration",
           "STATUS", "MAX_ITERATIONS"]

MAX_ITERATIONS = 1000                                                   # include/m3slam.h
STATUS = ("ok", "too_few_pairs", "singular")
_METHODS = {"point_to_point": 0, "point_to_plane": 1}
_STATE_WORDS, _HIST_WORDS = 24, 5

IcpSums = namedtuple("IcpSums", ["count", "H", "g", "cost", "pairs", "finite", "out_of_range"])
IcpSums.__doc__ = ("One linearisation: count = the contributing pairs; H float64 [7,7] and g float64 [7] over (translation, "
                   "rotation, scale); cost = the sum of squared residuals; pairs int32 [Ns] device tensor (-1: no "
                   "correspondence) or None; finite = the source rows that are finite after the move; out_of_range = those of "
                   "them whose grid cell reaches +-2^20.")


class Registration(namedtuple("Registration", ["T", "scale", "fitness", "inlier_rmse", "iterations", "converged", "status",
                                               "history", "pairs", "out_of_range"])):
    """T float64 [4,4] = [[s R, t], [0, 1]], source to target; scale = s; fitness = the source rows with a correspondence
    at T over the finite source rows; inlier_rmse over those pairs; iterations = those that ran; converged: the last step
    fell below tol; status: "ok", "too_few_pairs" or "singular" (the pose is the one before the failing iteration);
    history float64 [iterations,5]: pairs, cost, |translation step|^2, |rotation step|^2, scale step of each iteration;
    pairs int32 [Ns] device tensor - the target row of every source row at T, -1 without - or None; out_of_range: the
    finite source rows whose grid cell reaches +-2^20 at T (they match nothing)."""
    __slots__ = ()

    def apply(self, points: torch.Tensor) -> torch.Tensor:
        """The [n,3] points moved by T, in their own dtype (the product is formed in float64)."""
        if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
            raise ValueError("points must be an [n,3] tensor")
        T = torch.from_numpy(np.ascontiguousarray(self.T)).to(points.device)
        return (points.to(torch.float64) @ T[:3, :3].T + T[:3, 3]).to(points.dtype)


def registration_workspace_bytes(Ns: int, Nt: int, iterations: int = 30) -> int:
    """Bytes of the workspace of register_clouds (icp_sums: iterations = 0)."""
    b = int(_ffi.lib().m3_icp_ws_bytes(int(Ns), int(Nt), int(iterations)))
    if b <= 0:
        raise ValueError(f"unsupported registration of {Ns} onto {Nt} points in {iterations} iterations")
    return b


def _integer(v, name: str, lo: int, hi: int) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f"{name} must be an integer in {lo} ... {hi}, got {v!r}")
    return int(v)


def _pose(T) -> np.ndarray:
    """double [13] = R | t | s of a 4 x 4 with s R | t; ValueError unless R is a rotation to 1e-6."""
    if T is None:
        return np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1], np.float64)
    if isinstance(T, torch.Tensor):
        T = T.detach().cpu().numpy()
    M = np.asarray(T, dtype=np.float64)
    if M.shape != (4, 4) or not np.isfinite(M).all():
        raise ValueError("T must be a finite 4 x 4 matrix")
    if not np.array_equal(M[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError("the last row of T must be 0 0 0 1")
    s = math.sqrt(float(M[0, 0]) ** 2 + float(M[1, 0]) ** 2 + float(M[2, 0]) ** 2)
    if not s > 0.0:
        raise ValueError("T has no scale: its first column is zero")
    R = M[:3, :3] / s
    if np.abs(R.T @ R - np.eye(3)).max() > 1e-6 or not np.linalg.det(R) > 0.0:
        raise ValueError("T must be a similarity: s R | t with R a rotation (R^T R = I to 1e-6, det > 0)")
    return np.concatenate([R.reshape(9), M[:3, 3], [s]])


def _clouds(source, target, radius, target_normals, method):
    """(r, mode) after every check that needs no device."""
    r, _ = _radius(radius)
    _points(source, "source")
    _points(target, "target")
    if target_normals is not None:
        _points(target_normals, "target_normals")
        if target_normals.shape[0] != target.shape[0]:
            raise ValueError(f"{target.shape[0]} target points, {target_normals.shape[0]} normals")
    if method is None:
        method = "point_to_plane" if target_normals is not None else "point_to_point"
    if method not in _METHODS:
        raise ValueError(f"method must be one of {sorted(_METHODS)}, got {method!r}")
    if method == "point_to_plane" and target_normals is None:
        raise ValueError("point_to_plane needs target_normals")
    return r, _METHODS[method]


def _on_device(source, target, target_normals):
    source = _ffi.check(source, torch.float32, "source")
    target = _ffi.check(target, torch.float32, "target")
    dev = source.device
    if target_normals is not None:
        target_normals = _ffi.check(target_normals, torch.float32, "target_normals")
    if target.device != dev or (target_normals is not None and target_normals.device != dev):
        raise ValueError(f"the source lives on {dev}, the target on {target.device}")
    return source, target, target_normals


def _workspace(workspace, ns, nt, iterations, dev):
    return take_workspace(workspace, registration_workspace_bytes(ns, nt, iterations), dev, owner="the clouds live")


def _state_offset(nt: int) -> int:
    return (int(_ffi.lib().m3_cloud_ws_bytes(int(nt))) + 15) // 16 * 16


def icp_sums(source, target, radius, T, target_normals=None, method=None, return_pairs: bool = False) -> IcpSums:
    """IcpSums of one linearisation at the pose T (4 x 4, s R | t; None: the identity): what one iteration of
    register_clouds adds up, for tests and for callers with a solver of their own.  8 launches, one read.  ValueError and
    RuntimeError as register_clouds."""
    r, mode = _clouds(source, target, radius, target_normals, method)
    pose = _pose(T)
    source, target, target_normals = _on_device(source, target, target_normals)
    ns, nt, dev = int(source.shape[0]), int(target.shape[0]), source.device
    ws = _workspace(None, ns, nt, 0, dev)
    out = torch.empty((3 + 36,), dtype=torch.float64, device=dev)       # int64 [3] | double [36]
    pairs = torch.empty((ns,), dtype=torch.int32, device=dev) if return_pairs else None
    host = (ctypes.c_double * 13)(*pose.tolist())
    _ffi.call("m3_icp_sums", _ffi.ptr(source), ns, _ffi.ptr(target), _ffi.ptr(target_normals), nt, r, mode,
              ctypes.addressof(host), out.data_ptr(), out.data_ptr() + 24, _ffi.ptr(pairs), _ffi.ptr(ws), ws.numel(),
              _ffi.stream_ptr())
    got = out.cpu()
    count = got[:3].view(torch.int64).tolist()
    s = got[3:].numpy()
    H = np.zeros((7, 7))
    H[np.triu_indices(7)] = s[:28]
    H = H + np.triu(H, 1).T
    return IcpSums(count[0], H, s[28:35].copy(), float(s[35]), pairs, count[1], count[2])


def read_registration(workspace: torch.Tensor, Ns: int, Nt: int, iterations: int, pairs=None) -> Registration:
    """The Registration a finished register_clouds call left in its workspace: one read of state and history.  For a call
    that was captured into a graph, after a replay."""
    at = _state_offset(Nt)
    words = _STATE_WORDS + _HIST_WORDS * int(iterations)
    raw = workspace[at:at + 8 * words].view(torch.float64).cpu().numpy()
    st, hist = raw[:_STATE_WORDS], raw[_STATE_WORDS:].reshape(-1, _HIST_WORDS)
    T = np.eye(4)
    T[:3, :3] = st[12] * st[:9].reshape(3, 3)
    T[:3, 3] = st[9:12]
    ran, ev_pairs, finite = int(st[13]), float(st[20]), float(st[18])
    return Registration(T, float(st[12]), ev_pairs / finite if finite else 0.0,
                        math.sqrt(float(st[21]) / ev_pairs) if ev_pairs else 0.0, ran, bool(st[14]), STATUS[int(st[15])],
                        hist[:ran].copy(), pairs, int(st[19]))


def register_clouds(source, target, radius, target_normals=None, method=None, T_init=None, with_scale: bool = False,
                    iterations: int = 30, tol: float = 1e-6, min_pairs: int = 16, return_pairs: bool = False,
                    workspace: Optional[torch.Tensor] = None) -> Registration:
    """Registration of the float32 [Ns,3] device tensor `source` onto the float32 [Nt,3] `target`: T with T source ~ target.

    radius: how far a correspondence may be - a few voxel edges of a thinned cloud; a source point with no target point
    within it takes no part.  target_normals float32 [Nt,3] (cloud_normals of the target) select point to plane unless
    method says "point_to_point"; "point_to_plane" without normals is a ValueError.  T_init: a 4 x 4 similarity s R | t
    (numpy or tensor); s is the norm of its first column and R = M / s - ValueError when R^T R is off the identity by more
    than 1e-6 or det <= 0.  with_scale: also estimate the scale (Sim(3)); otherwise the scale of T_init is kept.
    iterations in 0 ... 1000, tol >= 0, min_pairs >= 1: this project's defaults, untuned on real data.  return_pairs: the
    final correspondence of every source row.

    Source rows that are not finite, rows far from the target and rows whose grid cell is out of range match nothing and
    are otherwise harmless; the latter are counted in out_of_range.  Identical bytes on every call.  6 + 2 * iterations +
    2 launches and one read at the end.  workspace: a 16-byte aligned uint8 device tensor of
    registration_workspace_bytes(Ns, Nt, iterations); with it the call can be captured into a graph - nothing is read then,
    every field but pairs is None, and read_registration gives the result after a replay.  ValueError before any device
    call for bad arguments; RuntimeError for CPU tensors."""
    r, mode = _clouds(source, target, radius, target_normals, method)
    pose = _pose(T_init)
    if not isinstance(with_scale, (bool, np.bool_)):
        raise ValueError(f"with_scale must be a bool, got {with_scale!r}")
    iterations = _integer(iterations, "iterations", 0, MAX_ITERATIONS)
    min_pairs = _integer(min_pairs, "min_pairs", 1, 2 ** 62)
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or not math.isfinite(tol) or tol < 0:
        raise ValueError(f"tol must be a finite number >= 0, got {tol!r}")
    source, target, target_normals = _on_device(source, target, target_normals)
    ns, nt, dev = int(source.shape[0]), int(target.shape[0]), source.device
    ws = _workspace(workspace, ns, nt, iterations, dev)
    pairs = torch.empty((ns,), dtype=torch.int32, device=dev) if return_pairs else None
    host = (ctypes.c_double * 13)(*pose.tolist())
    _ffi.call("m3_icp_register", _ffi.ptr(source), ns, _ffi.ptr(target), _ffi.ptr(target_normals), nt, r, mode,
              ctypes.addressof(host), int(bool(with_scale)), iterations, float(tol), min_pairs, _ffi.ptr(pairs), _ffi.ptr(ws),
              ws.numel(), _ffi.stream_ptr())
    if torch.cuda.is_current_stream_capturing():
        return Registration(None, None, None, None, None, None, None, None, pairs, None)
    return read_registration(ws, ns, nt, iterations, pairs)
