"""Volumetric fusion of the keyframe map, on the device (csrc/tsdf.hip).

collect_map and collect_mesh emit every keyframe's pointmap as its own layer: where keyframes overlap, the cloud holds N
noisy copies of the surface and the mesh N sheets that share no vertex.  fuse_tsdf averages the pointmaps into one
truncated signed distance field on a dense voxel grid, and extract_surface takes one connected triangle mesh out of it
(naive surface nets: one vertex per cell the surface crosses, one quad per grid edge it crosses), watertight wherever
the volume is observed.

    D[j][m]            X_j[m].z where (j, m) passes the confidence test, z is finite and z > z_min, else NaN (the
                       consistency filter's observation plane)
    voxel centre p     origin + (index + 0.5) * voxel_size
    per keyframe j     c = R_j^T (p - t_j) / s_j, needs c.z > z_min; pixel floor(fx c.x / c.z + cx + 0.5),
                       floor(fy c.y / c.z + cy + 0.5) inside the H x W grid; d = D[j][pixel], NaN: no observation;
                       sdf = (d - c.z) * s_j, needs sdf >= -trunc (else the voxel is occluded in j);
                       sum += min(sdf / trunc, 1), n += 1; sdf <= trunc: the pixel's colour is added too
    tsdf, weight       sum / n (1 where n = 0), n;  color: the rounded mean of the added colours
    surface            cells whose 8 corner voxels have weight >= min_weight and tsdf values of both signs

The exact rules, with the order of every operation, are in include/m3slam.h.  Approximations: the sdf is projective
(along the camera's z) with nearest-pixel depth; the pointmap is treated as a depth image of the pinhole K (the
consistency filter's approximation: exact when the points lie on the rays of K); weights are counts, not confidences.

This is a batch pass over the CURRENT keyframes and their current, backend-optimised poses, not an incremental
integration inside the loop (which would bake stale poses into the volume): it is opt-in and nothing in the loop calls
it.  One fuse_tsdf call queues three launches whatever the number of keyframes and voxels, reads nothing back given
`out`, `workspace` and explicit `bounds`, and can be captured into a graph (poses are read on the device).  Two calls
give identical bytes.  CPU tensors raise RuntimeError: there is no CPU path.

The defaults - trunc = 4 * voxel_size, 256 voxels along the longest side in SLAM.fused_mesh, min_weight = 1 - are this
project's choice, like c_conf_threshold: nobody has tuned them on real data.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _ffi
from ._mesh_args import take_workspace
from ._view_args import _check_K_word, _map_frames, map_camera, planes_workspace_bytes
from .export import _MapTables, _conf_gate, _empty_mesh, collect_map

__all__ = ["fuse_tsdf", "extract_surface", "TSDFVolume", "volume_grid", "empty_volume", "map_bounds"]

MIN_DIM, MAX_DIM, MAX_VOXELS = 2, 1024, 1 << 30                        # include/m3slam.h
MAX_EXTRACT_VOXELS = (2 ** 31 - 1) // 3                                # face-yielding edges are counted in int32


@dataclass
class TSDFVolume:
    """tsdf float32 [Dz,Dy,Dx], weight int32 [Dz,Dy,Dx] (observations per voxel), color uint8 [Dz,Dy,Dx,3], colored uint8
    [Dz,Dy,Dx] (1 where an observation within the truncation band gave the voxel a colour; None: everywhere) as device
    tensors; origin: the low corner of voxel (0, 0, 0) as three fp32 values (x, y, z); voxel_size and trunc as fp32
    values."""
    tsdf: torch.Tensor
    weight: torch.Tensor
    color: torch.Tensor
    origin: tuple
    voxel_size: float
    trunc: float
    colored: Optional[torch.Tensor] = None

    @property
    def dims(self) -> tuple:
        """(Dz, Dy, Dx)."""
        return tuple(int(d) for d in self.tsdf.shape)


def _f32(v) -> float:
    return float(np.float32(v))


def _sizes(voxel_size, trunc):
    vs = _f32(voxel_size)
    if not (0.0 < vs < math.inf):
        raise ValueError(f"voxel_size must be positive and finite, got {voxel_size}")
    tr = _f32(4.0 * vs if trunc is None else trunc)
    if not (0.0 < tr < math.inf):
        raise ValueError(f"trunc must be positive and finite, got {trunc}")
    return vs, tr


def _grid(bounds, vs: float, tr: float):
    lo, hi = (np.asarray(b, dtype=np.float64).reshape(-1) for b in bounds)
    if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all()) or (hi < lo).any():
        raise ValueError(f"bounds must be two finite (x, y, z) corners with hi >= lo, got {bounds!r}")
    pad = tr + vs
    origin = np.floor((lo - pad) / vs) * vs
    dims = np.maximum(np.ceil((hi + pad - origin) / vs), MIN_DIM)
    return origin.astype(np.float32), dims


def _dims_ok(dims) -> bool:
    return bool((dims >= MIN_DIM).all() and (dims <= MAX_DIM).all() and float(np.prod(dims)) <= MAX_VOXELS)


def volume_grid(bounds, voxel_size: float, trunc: Optional[float] = None):
    """(origin fp32 [3] as (x, y, z), (Dz, Dy, Dx)) of the volume fuse_tsdf lays over bounds = (lo, hi): the box is padded by
    trunc + voxel_size on every side, the origin is snapped down to a multiple of the voxel size (computed in float64,
    rounded to fp32) and the dims cover the padded box.  ValueError when a dim leaves 2 ... 1024 or the volume 2^30
    voxels; the message names a voxel size that fits."""
    vs, tr = _sizes(voxel_size, trunc)
    origin, dims = _grid(bounds, vs, tr)
    if not _dims_ok(dims):
        fit = vs
        for _ in range(2000):                                          # 5 % steps: the first size whose grid fits
            fit *= 1.05
            if _dims_ok(_grid(bounds, _f32(fit), _f32(4.0 * fit) if trunc is None else tr)[1]):
                break
        raise ValueError(f"voxel_size {vs:g} gives a volume of {int(dims[0])} x {int(dims[1])} x {int(dims[2])} voxels (x, y, z); "
                         f"each side must lie in {MIN_DIM} ... {MAX_DIM} and the volume within 2^30 voxels: a voxel_size of "
                         f"{_f32(fit):g} would fit")
    return origin, (int(dims[2]), int(dims[1]), int(dims[0]))


def empty_volume(origin, dims, voxel_size: float, trunc: Optional[float] = None, device="cuda") -> TSDFVolume:
    """An uninitialised volume of dims = (Dz, Dy, Dx) with its low corner at origin (x, y, z): pass it as fuse_tsdf's `out`
    to fix the grid without bounds."""
    vs, tr = _sizes(voxel_size, trunc)
    d = np.asarray([int(v) for v in dims], dtype=np.float64)
    o = np.asarray(origin, dtype=np.float64).reshape(-1)
    if d.shape != (3,) or not _dims_ok(d):
        raise ValueError(f"dims must be (Dz, Dy, Dx), each in {MIN_DIM} ... {MAX_DIM}, with at most 2^30 voxels, got {tuple(dims)}")
    if o.shape != (3,) or not np.isfinite(o.astype(np.float32)).all():
        raise ValueError(f"origin must be three finite values, got {origin!r}")
    shape = tuple(int(v) for v in dims)
    return TSDFVolume(torch.empty(shape, dtype=torch.float32, device=device), torch.empty(shape, dtype=torch.int32, device=device),
                      torch.empty(shape + (3,), dtype=torch.uint8, device=device), tuple(_f32(v) for v in o), vs, tr,
                      torch.empty(shape, dtype=torch.uint8, device=device))


def map_bounds(keyframes, c_conf_threshold: Optional[float] = 1.5):
    """(lo, hi) of collect_map's points under the same threshold: device amin / amax and one host read.  ValueError when
    the map has no point."""
    frames = keyframes.frames if isinstance(keyframes, _MapTables) else keyframes
    points = collect_map(frames, c_conf_threshold=c_conf_threshold)[0]
    if points.shape[0] == 0:
        raise ValueError("the map has no point under this threshold: pass bounds")
    box = torch.stack([points.amin(dim=0), points.amax(dim=0)]).cpu().numpy().astype(np.float64)
    return box[0], box[1]


def workspace_bytes(k: int, n: int) -> int:
    """Bytes of the inverse-pose table and the observation planes fuse_tsdf needs for k keyframes of n pixels."""
    return planes_workspace_bytes("m3_tsdf_integrate_ws_bytes", k, n)


def _check_volume(v: TSDFVolume, shape, need_colored: bool) -> None:
    if not isinstance(v, TSDFVolume):
        raise TypeError(f"expected a TSDFVolume, got {type(v).__name__}")
    for t, dt, name, sh in ((v.tsdf, torch.float32, "tsdf", shape), (v.weight, torch.int32, "weight", shape),
                            (v.color, torch.uint8, "color", shape + (3,)), (v.colored, torch.uint8, "colored", shape)):
        if t is None and name == "colored" and not need_colored:
            continue
        if _ffi.check(t, dt, f"volume {name}", sh).data_ptr() != t.data_ptr() or t.data_ptr() % 4:
            raise ValueError(f"volume {name} must be contiguous and 4-byte aligned")


def fuse_tsdf(keyframes, K, voxel_size: float, bounds=None, trunc: Optional[float] = None,
              c_conf_threshold: Optional[float] = 1.5, z_min: float = 1e-3, out: Optional[TSDFVolume] = None,
              workspace: Optional[torch.Tensor] = None) -> TSDFVolume:
    """The TSDFVolume of `keyframes` by the rule at the top of this module.

    keyframes and K as consistency.multiview_support takes them (a Keyframes, a sequence of frames or ConsistentFrame
    views, the result of render.map_tables; a 3 x 3 matrix, (fx, fy, cx, cy) or "estimate").  trunc None: 4 * voxel_size.
    bounds: (lo, hi), two (x, y, z) corners; the volume is volume_grid(bounds, voxel_size, trunc).  bounds None: out's own
    grid when `out` is given, else map_bounds(keyframes, c_conf_threshold) - collect_map's points under the same
    threshold, which costs that export and one host read.  c_conf_threshold None: no confidence test.

    out: a TSDFVolume to write into (empty_volume); with bounds, its grid must be the one the bounds give.  workspace: a
    16-byte aligned uint8 device tensor of workspace_bytes(K, N).  With out, workspace and explicit bounds (or out's own
    grid) nothing is read back and nothing is allocated in the library.  Poses are gathered from the frames' T_WC
    tensors on the device on every call, so a captured call follows poses that are updated in place.

    No keyframes: the unobserved volume (tsdf 1, weight 0), which needs bounds or out.  ValueError - before anything is
    launched - for a voxel_size / trunc that is not positive and finite, a negative z_min, dims outside 2 ... 1024 or a
    volume beyond 2^30 voxels (the message names a voxel size that fits), keyframes of different image sizes; RuntimeError
    for CPU tensors."""
    vs, tr = _sizes(voxel_size, trunc)
    z_min = float(z_min)
    if not 0.0 <= z_min < math.inf:
        raise ValueError(f"z_min must be >= 0 and finite, got {z_min}")
    frames = _map_frames(keyframes)
    _check_K_word(K)                                                   # before the grid: the order this call has always had
    if bounds is not None:
        origin, shape = volume_grid(bounds, vs, tr)
        origin = tuple(float(v) for v in origin)
    elif out is not None:
        if not isinstance(out, TSDFVolume):
            raise TypeError(f"out must be a TSDFVolume, got {type(out).__name__}")
        origin, shape = tuple(_f32(v) for v in out.origin), out.dims
    else:
        origin = None                                                  # from the map, once the tables exist
    if out is not None and (not isinstance(out, TSDFVolume) or tuple(_f32(v) for v in out.origin) != origin or
                            out.dims != tuple(shape) or _f32(out.voxel_size) != vs or _f32(out.trunc) != tr):
        raise ValueError(f"out must be a TSDFVolume of this call's grid: origin {origin}, dims {tuple(shape)}, voxel_size {vs}, "
                         f"trunc {tr}; the call asks for another one than out has")
    m, (h, w), (fx, fy, cx, cy), poses = map_camera(keyframes, frames, K, c_conf_threshold)
    if origin is None:
        if m is None:
            raise ValueError("no keyframes: the volume needs bounds or out")
        origin, shape = volume_grid(map_bounds(m, c_conf_threshold), vs, tr)
        origin = tuple(float(v) for v in origin)
    dev = m.device if m is not None else (out.tsdf.device if out is not None else torch.device("cuda"))
    if out is None:
        out = empty_volume(origin, shape, vs, tr, dev)
    else:
        _check_volume(out, tuple(shape), need_colored=False)
    k = m.k if m is not None else 0
    use, thr = _conf_gate(c_conf_threshold)
    dz, dy, dx = shape
    if k:
        ws_bytes = workspace_bytes(k, m.n)
        workspace = take_workspace(workspace, ws_bytes, dev, owner=None)
        tables = (_ffi.ptr(m.table[0]), _ffi.ptr(m.table[1]), _ffi.ptr(m.table[2]), _ffi.ptr(poses), _ffi.ptr(m.nk))
        layout = m.layout
    else:
        ws_bytes, workspace, tables, layout = 0, None, (None,) * 5, 1
    _ffi.call("m3_tsdf_integrate", *tables, k, h, w, use, thr, layout, fx, fy, cx, cy, z_min, origin[0], origin[1], origin[2],
              vs, tr, dx, dy, dz, _ffi.ptr(workspace), ws_bytes, _ffi.ptr(out.tsdf), _ffi.ptr(out.weight), _ffi.ptr(out.color),
              _ffi.ptr(out.colored), _ffi.stream_ptr())
    return out


def extract_surface(volume: TSDFVolume, min_weight: int = 1):
    """(vertices float32 [V,3], colors uint8 [V,3], faces int32 [F,3]) of the surface tsdf = 0 of `volume`, as device
    tensors: one vertex per cell whose 8 corner voxels have weight >= min_weight and tsdf values of both signs, in
    ascending (z, y, x); two triangles per grid edge whose ends differ in sign and whose four surrounding cells are
    active, in ascending (z, y, x, direction), with normals towards the free-space side.  Every face references vertices
    of this mesh; a volume whose surface gives no face gives an empty mesh.  The host reads V and F once, between the
    count and the scatter.  ValueError for min_weight < 1 or a volume of more than (2^31 - 1) / 3 voxels (edges are
    counted in int32); RuntimeError for CPU tensors."""
    if isinstance(min_weight, bool) or int(min_weight) != min_weight or min_weight < 1:
        raise ValueError(f"min_weight must be an integer >= 1, got {min_weight}")
    if not isinstance(volume, TSDFVolume):
        raise TypeError(f"expected a TSDFVolume, got {type(volume).__name__}")
    shape = volume.dims
    if len(shape) != 3 or not _dims_ok(np.asarray(shape, dtype=np.float64)):
        raise ValueError(f"volume dims must be (Dz, Dy, Dx), each in {MIN_DIM} ... {MAX_DIM}, got {shape}")
    dz, dy, dx = shape
    if dz * dy * dx > MAX_EXTRACT_VOXELS:
        raise ValueError(f"a volume of {dz * dy * dx} voxels is too large for one extraction (limit {MAX_EXTRACT_VOXELS})")
    vs = _f32(volume.voxel_size)
    origin = tuple(_f32(v) for v in volume.origin)
    if not (0.0 < vs < math.inf) or len(origin) != 3 or not all(math.isfinite(v) for v in origin):
        raise ValueError(f"volume needs a positive voxel_size and a finite origin, got {volume.voxel_size}, {volume.origin}")
    _check_volume(volume, shape, need_colored=False)
    dev = volume.tsdf.device
    L = _ffi.lib()
    ws_bytes = int(L.m3_tsdf_extract_ws_bytes(dx, dy, dz))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    st = _ffi.stream_ptr()
    _ffi.call("m3_tsdf_extract_count", _ffi.ptr(volume.tsdf), _ffi.ptr(volume.weight), dx, dy, dz, int(min_weight), _ffi.ptr(ws),
              ws_bytes, st)
    v, e = ws[:8].view(torch.int32).tolist()                            # the one synchronisation: V and F / 2 in one copy
    if e == 0:
        return _empty_mesh(dev, False)
    f = 2 * e
    vertices = torch.empty((v, 3), dtype=torch.float32, device=dev)
    colors = torch.empty((v, 3), dtype=torch.uint8, device=dev)
    faces = torch.empty((f, 3), dtype=torch.int32, device=dev)
    _ffi.call("m3_tsdf_extract_scatter", _ffi.ptr(volume.tsdf), _ffi.ptr(volume.weight), _ffi.ptr(volume.color),
              _ffi.ptr(volume.colored), origin[0], origin[1], origin[2], vs, dx, dy, dz, int(min_weight), _ffi.ptr(ws), ws_bytes,
              v, f, _ffi.ptr(vertices), _ffi.ptr(colors), _ffi.ptr(faces), st)
    return vertices, colors, faces
