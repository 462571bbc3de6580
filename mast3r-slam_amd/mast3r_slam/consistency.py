"""Multi-view consistency filter for the keyframe map, on the device (csrc/consistency.hip).

collect_map, collect_mesh and render_map keep a point when its own keyframe's average confidence passes a threshold.
This module adds the cross-check every dense reconstruction pipeline makes: a point survives when enough OTHER keyframes
saw the same surface there and not too many saw through it.

    D[j][m]          X_j[m].z where (j, m) passes the confidence test, z is finite and z > z_min, else NaN: keyframe j's
                     observed depth at pixel m (X_canon is in j's camera frame)
    candidate(k, n)  export.collect_map's rule: C[k][n] / N_k > c_conf_threshold (None: no test), world point finite
    per neighbour j  c = R_j^T (p - t_j) / s_j (the renderer's camera point), needs c.z > z_min;
                     pixel floor(fx c.x / c.z + cx + 0.5), floor(fy c.y / c.z + cy + 0.5) inside the H x W grid;
                     d = D[j][pixel], NaN: j has no observation there;
                     |c.z - d| <= depth_rtol * d: support + 1;  else c.z < d: conflict + 1 (j saw through the point);
                     else nothing (the point is occluded in j)
    kept             candidate and support >= min_views and (max_conflicts is None or conflict <= max_conflicts)
    conf[k][n]       C[k][n] when kept, else -inf

The masked confidence is the integration point: consistent_keyframes wraps the keyframes in views whose C is a row of
`conf`, and every consumer of keyframes (collect_map, collect_mesh, render_map, estimate_focal), under the same or any
other finite threshold, then drops exactly the rejected points.

One call queues three launches whatever the number of keyframes, neighbours or pixels, reads nothing back and, given
`out` and `workspace`, allocates nothing in the library; poses are read on the device, so the call can be captured
into a graph.  Two calls give identical bytes.  CPU tensors raise RuntimeError: there is no CPU path.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import _ffi
from ._mesh_args import take_workspace
from ._view_args import _map_frames, map_camera, planes_workspace_bytes
from .export import _conf_gate

__all__ = ["multiview_support", "consistent_keyframes", "nearest_neighbours", "ConsistentFrame"]

MAX_NEIGHBOURS = 255                                                   # include/m3slam.h: the counts are uint8


def _scalars(depth_rtol, min_views, max_conflicts, z_min):
    depth_rtol, z_min = float(depth_rtol), float(z_min)
    if not 0.0 < depth_rtol < 1.0:
        raise ValueError(f"depth_rtol must lie in (0, 1), got {depth_rtol}")
    if isinstance(min_views, bool) or int(min_views) != min_views or min_views < 0:
        raise ValueError(f"min_views must be an integer >= 0, got {min_views}")
    if max_conflicts is not None and (isinstance(max_conflicts, bool) or int(max_conflicts) != max_conflicts or max_conflicts < 0):
        raise ValueError(f"max_conflicts must be None or an integer >= 0, got {max_conflicts}")
    if not 0.0 <= z_min < math.inf:
        raise ValueError(f"z_min must be >= 0 and finite, got {z_min}")
    return depth_rtol, int(min_views), -1 if max_conflicts is None else int(max_conflicts), z_min


def _check_neighbours(neighbours):
    """The shape-only part of the neighbour argument: ValueError before anything touches a device."""
    if neighbours is None:
        return
    if isinstance(neighbours, torch.Tensor):
        if neighbours.dim() != 2:
            raise ValueError(f"neighbours must be an int32 [K,V] tensor, got shape {tuple(neighbours.shape)}")
        v = int(neighbours.shape[1])
    else:
        if isinstance(neighbours, bool) or int(neighbours) != neighbours or neighbours < 0:
            raise ValueError(f"neighbours must be None, an integer >= 0 or an int32 [K,V] tensor, got {neighbours!r}")
        v = int(neighbours)
    if v > MAX_NEIGHBOURS:
        raise ValueError(f"at most {MAX_NEIGHBOURS} neighbours per keyframe (the counts are uint8), got V = {v}")


def nearest_neighbours(poses: torch.Tensor, v: int) -> torch.Tensor:
    """int32 [K, min(v, K - 1)]: for every row of poses [K,8] the other keyframes with the nearest camera centres, nearest
    first, computed on the device without a host read: fp32 squared distances ((tx_i - tx_j)^2 + (ty_i - ty_j)^2) +
    (tz_i - tz_j)^2, the diagonal set to +inf, a stable ascending sort, the first columns."""
    k = int(poses.shape[0])
    v = min(int(v), k - 1)
    if v <= 0:
        return torch.empty((k, 0), dtype=torch.int32, device=poses.device)
    t = poses[:, :3].to(torch.float32)
    d = t[:, None, :] - t[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    d2 = d2.masked_fill(torch.eye(k, dtype=torch.bool, device=poses.device), math.inf)
    return torch.sort(d2, dim=1, stable=True).indices[:, :v].to(torch.int32).contiguous()


def _all_others(k: int, dev) -> torch.Tensor:
    """int32 [K, K - 1]: row i lists every keyframe but i, ascending.  Built on the device."""
    j = torch.arange(max(k - 1, 0), device=dev, dtype=torch.int32)[None, :]
    return (j + (j >= torch.arange(k, device=dev, dtype=torch.int32)[:, None]).to(torch.int32)).contiguous()


def workspace_bytes(k: int, n: int) -> int:
    """Bytes of the inverse-pose table and the observation planes multiview_support needs for k keyframes of n pixels."""
    return planes_workspace_bytes("m3_consistency_ws_bytes", k, n)


def multiview_support(keyframes, K, neighbours=8, c_conf_threshold: Optional[float] = 1.5, depth_rtol: float = 0.03,
                      min_views: int = 2, max_conflicts: Optional[int] = 1, z_min: float = 1e-3, out=None,
                      workspace: Optional[torch.Tensor] = None):
    """(support uint8 [K,N], conflict uint8 [K,N], conf float32 [K,N]) of `keyframes` (as collect_map takes them, or the
    result of render.map_tables), as device tensors, by the rule at the top of this module.

    K: the pinhole of the keyframes' own H x W grid: a 3 x 3 tensor / array, an (fx, fy, cx, cy) tuple, or "estimate"
    (intrinsics.estimate_intrinsics(keyframes): that function's one read-back).
    neighbours: None - every other keyframe; an int V - the min(V, K - 1) other keyframes with the nearest camera
    centres (nearest_neighbours, on the device); an int32 [K,V] device tensor - used as given, -1 = none, an entry that
    names its own row or no keyframe is skipped.  V <= 255.
    c_conf_threshold None: no confidence test, for sources and observation planes alike.  max_conflicts None: no
    limit.  The defaults (depth_rtol 0.03, min_views 2, max_conflicts 1, 8 neighbours) are this project's choice, like
    c_conf_threshold and the mesh's edge_ratio: nobody has tuned them on real data.

    Poses are gathered from the frames' T_WC tensors on the device on every call, so a captured call follows poses that
    are updated in place.  `out`: the three tensors to write into; `workspace`: a 16-byte aligned uint8 device tensor of
    workspace_bytes(K, N).  ValueError - before anything is launched - for V > 255, depth_rtol outside (0, 1), a
    negative min_views / max_conflicts / z_min, keyframes of different image sizes or a pointmap whose N != H * W;
    RuntimeError for CPU tensors.  No keyframes: three empty [0,0] tensors."""
    rtol, mv, mc, z_min = _scalars(depth_rtol, min_views, max_conflicts, z_min)
    _check_neighbours(neighbours)
    frames = _map_frames(keyframes)
    if not frames:
        dev = "cuda" if torch.cuda.is_available() else "cpu"
        return (torch.empty((0, 0), dtype=torch.uint8, device=dev), torch.empty((0, 0), dtype=torch.uint8, device=dev),
                torch.empty((0, 0), dtype=torch.float32, device=dev))
    m, (h, w), (fx, fy, cx, cy), poses = map_camera(keyframes, frames, K, c_conf_threshold)
    k, n, dev = m.k, m.n, m.device
    if neighbours is None:
        if k - 1 > MAX_NEIGHBOURS:
            raise ValueError(f"neighbours=None needs V = {k - 1} > {MAX_NEIGHBOURS}: pass a number of nearest neighbours")
        nbr = _all_others(k, dev)
    elif isinstance(neighbours, torch.Tensor):
        nbr = _ffi.check(neighbours, torch.int32, "neighbours", (k, None))
    else:
        nbr = nearest_neighbours(poses, int(neighbours))
    v = int(nbr.shape[1])
    ws_bytes = workspace_bytes(k, n)
    if out is None:
        out = (torch.empty((k, n), dtype=torch.uint8, device=dev), torch.empty((k, n), dtype=torch.uint8, device=dev),
               torch.empty((k, n), dtype=torch.float32, device=dev))
    if len(out) != 3:
        raise ValueError("out must hold support, conflict and conf")
    for t, dt, name in zip(out, (torch.uint8, torch.uint8, torch.float32), ("support", "conflict", "conf")):
        if _ffi.check(t, dt, f"out {name}", (k, n)).data_ptr() != t.data_ptr() or t.data_ptr() % 16:
            raise ValueError(f"out {name} must be contiguous and 16-byte aligned")
    workspace = take_workspace(workspace, ws_bytes, dev, owner=None)
    use, thr = _conf_gate(c_conf_threshold)
    _ffi.call("m3_consistency", _ffi.ptr(m.table[0]), _ffi.ptr(m.table[1]), _ffi.ptr(poses), _ffi.ptr(m.nk), k, h, w, use, thr,
              fx, fy, cx, cy, _ffi.ptr(nbr) if v else None, v, z_min, rtol, mv, mc, _ffi.ptr(workspace), ws_bytes,
              _ffi.ptr(out[0]), _ffi.ptr(out[1]), _ffi.ptr(out[2]), _ffi.stream_ptr())
    return tuple(out)


class ConsistentFrame:
    """A keyframe as the map consumers read it (frame_id, img, X_canon, T_WC, N, K, C), sharing the original's tensors
    except C, which is a row of multiview_support's masked confidence.  The original frame is not modified."""
    __slots__ = ("frame_id", "img", "X_canon", "T_WC", "N", "K", "C")

    def __init__(self, frame, conf: torch.Tensor) -> None:
        self.frame_id, self.img, self.X_canon, self.T_WC, self.N = frame.frame_id, frame.img, frame.X_canon, frame.T_WC, frame.N
        self.K = getattr(frame, "K", None)
        self.C = conf

    def get_average_conf(self) -> Optional[torch.Tensor]:
        return self.C / self.N if self.C is not None else None


def consistent_keyframes(keyframes, K, **kw) -> list:
    """The keyframes that have a pointmap as ConsistentFrame views whose C is the masked confidence of
    multiview_support(keyframes, K, **kw).  Anything that takes keyframes takes them: collect_map, collect_mesh,
    render_map, estimate_focal; a rejected point has confidence -inf and fails every finite threshold (pass -inf, not
    None, to mean "every kept point")."""
    frames = _map_frames(keyframes)
    conf = multiview_support(keyframes, K, **kw)[2]
    return [ConsistentFrame(f, conf[i].reshape(-1, 1)) for i, f in enumerate(frames)]
