"""Dense map export: what the reference's slam.py:320-415 (_get_results, save_trajectory, save_pointcloud) hands a user,
a coloured point cloud and a trajectory on disk.

collect_map gathers the world points and colours of every keyframe in ONE batched device pass (csrc/map_export.hip):
Sim(3) act, a test on the average confidence, the colour conversion and an ordered stream compaction, optionally
followed by voxel thinning.  The number of launches does not depend on the number of keyframes, the host reads one
integer (the kept count M) before it allocates exact-size outputs, and two calls give identical bytes.

    kept(k, n)  <=>  C[k][n] / N_k > c_conf_threshold   (fp32 divide as Frame.get_average_conf; strict; NaN fails)
                     and the world point s R X + t is finite
    order       =    ascending k * N + n
    colours     =    float [3,H,W]: (uint8)floor(clip(v, 0, 1) * 255), NaN -> 0;  uint8 [H,W,3]: passed through

`c_conf_threshold` defaults to 1.5, the value DEFAULT_CONFIG already uses for its Q_conf gates.  It is this project's
choice and a function argument, not a config key: the reference exports every point and has no such constant.  The
reference also writes ASCII PLY in a Python loop; here the body is one structured numpy array written in binary
(`binary=False` keeps the ASCII form for small clouds).  CPU tensors raise RuntimeError: there is no CPU path.

collect_mesh triangulates the same keyframes (csrc/mesh.hip): every pointmap is an organised
H x W grid, so each cell of neighbouring pixels gives two triangles, and a triangle is refused when an edge is long
against the range of its end points (a depth discontinuity).  Vertices are the exporter's world points and colours;
save_ply_mesh writes them with a face element.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import _ffi

__all__ = ["collect_map", "collect_mesh", "save_ply", "save_ply_mesh", "save_ply_mesh_normals", "save_ply_normals",
           "save_trajectory"]

IMG_F32_CHW, IMG_U8_HWC = 0, 1                                         # include/m3slam.h
_PLY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_PLY_NORMALS_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                               ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_PLY_FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])            # property list uchar int vertex_indices

last_voxel_stats: dict = {}           # table slots / occupied voxels of the most recent voxel pass (tools/bench_map_export.py)


def _empty(device, return_index: bool):
    out = (torch.empty((0, 3), dtype=torch.float32, device=device), torch.empty((0, 3), dtype=torch.uint8, device=device))
    return out + (torch.empty((0,), dtype=torch.int64, device=device),) if return_index else out


def _image(f, n: int):
    """(layout, contiguous image) of a frame; ValueError for anything but float32 [3,H,W] / uint8 [H,W,3] with H*W = n."""
    img = f.img
    if not isinstance(img, torch.Tensor) or img.dim() != 3:
        raise ValueError(f"frame {f.frame_id}: image must be a [3,H,W] float32 or [H,W,3] uint8 tensor")
    if img.dtype == torch.float32 and img.shape[0] == 3:
        layout, hw = IMG_F32_CHW, img.shape[1] * img.shape[2]
    elif img.dtype == torch.uint8 and img.shape[2] == 3:
        layout, hw = IMG_U8_HWC, img.shape[0] * img.shape[1]
    else:
        raise ValueError(f"frame {f.frame_id}: unsupported image {img.dtype} {tuple(img.shape)}; expected float32 [3,H,W] "
                         "or uint8 [H,W,3]")
    if hw != n:
        raise ValueError(f"frame {f.frame_id}: image has {hw} pixels, pointmap has {n} points")
    return layout, img


class _MapTables:
    """Device tables of per-keyframe pointers for csrc/map_export.hip and csrc/render.hip: table int64 [3,K] (X, C, image),
    nk int32 [K], poses float32 [K,8].  `hold` keeps the contiguous tensors alive until the launches are queued."""
    __slots__ = ("k", "n", "layout", "device", "table", "nk", "poses", "hold", "frames")


def _check_workspace(workspace: torch.Tensor, ws_bytes: int) -> None:
    """ValueError unless `workspace` is a contiguous, 16-byte aligned uint8 tensor of at least ws_bytes bytes."""
    _ffi.check(workspace, torch.uint8, "workspace")
    if workspace.numel() < ws_bytes or not workspace.is_contiguous() or workspace.data_ptr() % 16:
        raise ValueError(f"workspace must be a contiguous, 16-byte aligned uint8 tensor of at least {ws_bytes} bytes")


def _conf_gate(c_conf_threshold: Optional[float]):
    """(use_thresh, thresh) as the kernels take the confidence test; None: no test."""
    return (0, 0.0) if c_conf_threshold is None else (1, float(c_conf_threshold))


def _with_pointmap(keyframes) -> list:
    return [f for f in (keyframes._frames if hasattr(keyframes, "_frames") else list(keyframes)) if f.X_canon is not None]


def _map_tables(keyframes) -> Optional[_MapTables]:
    """Tables of `keyframes` (a Keyframes or a sequence of Frame; frames without a pointmap are skipped), None when no
    frame has a pointmap.  ValueError for mixed layouts / mismatched sizes or a map beyond 2^31 - 1 points, RuntimeError
    for CPU tensors."""
    frames = _with_pointmap(keyframes)
    if not frames:
        return None
    n = frames[0].X_canon.reshape(-1, 3).shape[0]
    layouts, hold = set(), []
    for f in frames:
        X = f.X_canon.reshape(-1, 3)
        if X.shape[0] != n:
            raise ValueError(f"frame {f.frame_id}: {X.shape[0]} points, the first keyframe has {n}")
        if f.C is None or f.C.numel() != n:
            raise ValueError(f"frame {f.frame_id}: confidence does not have one value per point")
        layout, img = _image(f, n)
        layouts.add(layout)
        hold.append((X, f.C.reshape(-1), img))
    if len(layouts) != 1:
        raise ValueError("keyframes mix float32 [3,H,W] and uint8 [H,W,3] images")
    m = _MapTables()
    m.frames, m.n, m.layout = frames, n, layouts.pop()
    m.device = dev = frames[0].X_canon.device
    # contiguous device tensors, kept alive until the launches are queued (the kernel takes scalar loads for a keyframe
    # whose arrays are not 16-byte aligned)
    m.hold = [(_ffi.check(X, torch.float32, "X_canon"), _ffi.check(C, torch.float32, "C"),
               _ffi.check(img, (torch.float32, torch.uint8), "img")) for X, C, img in hold]
    m.k = len(m.hold)
    if int(_ffi.lib().m3_map_export_ws_bytes(m.k, n)) <= 0:
        raise ValueError(f"map of {m.k} x {n} points is too large for one export (limit 2^31 - 1 points)")
    m.table = torch.tensor([[t.data_ptr() for t in col] for col in zip(*m.hold)], dtype=torch.int64).to(dev)   # [3,K]
    m.nk = torch.tensor([int(f.N) for f in frames], dtype=torch.int32).to(dev)
    m.poses = torch.cat([_ffi.check(f.T_WC.reshape(1, 8), torch.float32, "T_WC") for f in frames])
    return m


def collect_map(keyframes, c_conf_threshold: Optional[float] = 1.5, voxel_size: Optional[float] = None,
                return_index: bool = False):
    """World points float32 [M,3], colours uint8 [M,3] and (return_index) source indices int64 [M] of `keyframes`
    (a Keyframes or a sequence of Frame; frames without a pointmap are skipped), as device tensors.

    c_conf_threshold None keeps every finite point.  voxel_size > 0 keeps one point per occupied voxel
    floor(p / voxel_size): the one with the largest average confidence, ties to the smaller source index; ValueError
    when a voxel coordinate reaches 2^20 (voxel_size too small for the extent of the map)."""
    if voxel_size is not None and not float(voxel_size) > 0.0:
        raise ValueError(f"voxel_size must be positive, got {voxel_size}")
    m_ = _map_tables(keyframes)
    if m_ is None:
        return _empty("cuda" if torch.cuda.is_available() else "cpu", return_index)
    k, n, layout, dev, table, nk, poses = m_.k, m_.n, m_.layout, m_.device, m_.table, m_.nk, m_.poses
    L = _ffi.lib()
    ws_bytes = int(L.m3_map_export_ws_bytes(k, n))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    use, thr = _conf_gate(c_conf_threshold)
    st = _ffi.stream_ptr()
    _ffi.call("m3_map_export_count", _ffi.ptr(table[0]), _ffi.ptr(table[1]), _ffi.ptr(poses), _ffi.ptr(nk), k, n, use, thr,
              _ffi.ptr(ws), ws_bytes, st)
    m = int(ws[:4].view(torch.int32).item())                           # the one synchronisation of stage A
    if m == 0:
        return _empty(dev, return_index)
    thin = voxel_size is not None
    points = torch.empty((m, 3), dtype=torch.float32, device=dev)
    colors = torch.empty((m, 3), dtype=torch.uint8, device=dev)
    index = torch.empty((m,), dtype=torch.int64, device=dev) if return_index else None
    conf = torch.empty((m,), dtype=torch.float32, device=dev) if thin else None
    _ffi.call("m3_map_export_scatter", _ffi.ptr(table[0]), _ffi.ptr(table[1]), _ffi.ptr(table[2]), _ffi.ptr(poses),
              _ffi.ptr(nk), k, n, use, thr, layout, _ffi.ptr(ws), ws_bytes, m, _ffi.ptr(points), _ffi.ptr(colors),
              _ffi.ptr(index), _ffi.ptr(conf), st)
    if thin:
        points, colors, index = _voxel_thin(points, colors, index, conf, float(voxel_size))
    return (points, colors, index) if return_index else (points, colors)


def _voxel_thin(points, colors, index, conf, voxel_size: float):
    L = _ffi.lib()
    m, dev = points.shape[0], points.device
    ws_bytes = int(L.m3_map_voxel_ws_bytes(m))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    st = _ffi.stream_ptr()
    _ffi.call("m3_map_voxel_count", _ffi.ptr(points), _ffi.ptr(conf), m, voxel_size, _ffi.ptr(ws), ws_bytes, st)
    m2, dropped = ws[:8].view(torch.int32).tolist()
    if dropped:
        raise ValueError(f"voxel_size {voxel_size} is too small for this map: {dropped} points have a voxel coordinate "
                         "beyond +-2^20")
    last_voxel_stats.update(points=m, slots=int(L.m3_map_voxel_table_slots(m)), voxels=m2)
    p2 = torch.empty((m2, 3), dtype=torch.float32, device=dev)
    c2 = torch.empty((m2, 3), dtype=torch.uint8, device=dev)
    i2 = torch.empty((m2,), dtype=torch.int64, device=dev) if index is not None else None
    _ffi.call("m3_map_voxel_scatter", _ffi.ptr(points), _ffi.ptr(colors), _ffi.ptr(index), m, _ffi.ptr(ws), ws_bytes, m2,
              _ffi.ptr(p2), _ffi.ptr(c2), _ffi.ptr(i2), st)
    return p2, c2, i2


def _empty_mesh(device, return_index: bool):
    vertices, colors = _empty(device, False)
    out = (vertices, colors, torch.empty((0, 3), dtype=torch.int32, device=device))
    return out + (torch.empty((0,), dtype=torch.int64, device=device),) if return_index else out


def _grid_size(frames):
    """(H, W) of the frames' images; ValueError if they differ between keyframes."""
    first = None
    for f in frames:
        layout, img = _image(f, f.X_canon.reshape(-1, 3).shape[0])
        hw = tuple(img.shape[1:]) if layout == IMG_F32_CHW else tuple(img.shape[:2])
        first = first or hw
        if hw != first:
            raise ValueError(f"frame {f.frame_id}: image is {hw[0]}x{hw[1]}, the first keyframe's is {first[0]}x{first[1]}")
    return first


def collect_mesh(keyframes, c_conf_threshold: Optional[float] = 1.5, stride: int = 1, edge_ratio: Optional[float] = None,
                 return_index: bool = False):
    """Triangle mesh of `keyframes` (as collect_map takes them): vertices float32 [V,3], colours uint8 [V,3], faces
    int32 [F,3] and (return_index) source indices int64 [V], as device tensors.

    Every keyframe's pointmap is triangulated on its own pixel grid, every `stride`-th row and column: a cell of four
    neighbouring grid vertices a b / c d gives the triangles (a, c, b) and (b, c, d), counter-clockwise seen from the
    keyframe's camera.  A vertex is valid by collect_map's rule (c_conf_threshold None keeps every finite point).  An
    edge (p, q) passes when |p - q|^2 <= edge_ratio^2 * min(|p|^2, |q|^2) on the camera-frame points, a triangle is
    kept when its vertices are valid and its edges pass, and a vertex is emitted when a kept triangle references it.
    Vertices come in ascending source index k * H * W + y * W + x with the bytes collect_map gives that point; faces
    are rows of the vertex arrays in ascending (keyframe, grid row, grid column, triangle).  Meshes of overlapping
    keyframes are not merged.

    edge_ratio None means 0.02 * stride.  This is the project's choice, an argument like c_conf_threshold: at 512
    columns and roughly 60 degrees of view a fronto-parallel pixel step is about 0.0023 of the range, so 0.02 admits
    surfaces stretched about 6x the cell diagonal.  Nobody has tuned it on real data.

    ValueError for stride < 1, edge_ratio <= 0 or keyframes of different image sizes; RuntimeError for CPU tensors."""
    if int(stride) != stride or stride < 1:
        raise ValueError(f"stride must be a positive integer, got {stride}")
    stride = int(stride)
    ratio = 0.02 * stride if edge_ratio is None else float(edge_ratio)
    if not ratio > 0.0:
        raise ValueError(f"edge_ratio must be positive, got {edge_ratio}")
    frames = _with_pointmap(keyframes)
    if not frames:
        return _empty_mesh("cuda" if torch.cuda.is_available() else "cpu", return_index)
    h, w = _grid_size(frames)
    m_ = _map_tables(frames)
    k, dev, table = m_.k, m_.device, m_.table
    L = _ffi.lib()
    ws_bytes = int(L.m3_mesh_ws_bytes(k, h, w, stride))
    if ws_bytes <= 0:
        raise ValueError(f"{k} keyframes of {h}x{w} at stride {stride} are too many cells for one mesh (limit 2^30 - 1)")
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    use, thr = _conf_gate(c_conf_threshold)
    st = _ffi.stream_ptr()
    _ffi.call("m3_mesh_count", _ffi.ptr(table[0]), _ffi.ptr(table[1]), _ffi.ptr(m_.poses), _ffi.ptr(m_.nk), k, h, w, stride,
              use, thr, ratio, _ffi.ptr(ws), ws_bytes, st)
    v, f = ws[:8].view(torch.int32).tolist()                            # the one synchronisation: V and F in one copy
    if f == 0:
        return _empty_mesh(dev, return_index)
    vertices = torch.empty((v, 3), dtype=torch.float32, device=dev)
    colors = torch.empty((v, 3), dtype=torch.uint8, device=dev)
    faces = torch.empty((f, 3), dtype=torch.int32, device=dev)
    index = torch.empty((v,), dtype=torch.int64, device=dev) if return_index else None
    _ffi.call("m3_mesh_scatter", _ffi.ptr(table[0]), _ffi.ptr(table[1]), _ffi.ptr(table[2]), _ffi.ptr(m_.poses),
              _ffi.ptr(m_.nk), k, h, w, stride, use, thr, ratio, m_.layout, _ffi.ptr(ws), ws_bytes, v, f, _ffi.ptr(vertices),
              _ffi.ptr(colors), _ffi.ptr(faces), _ffi.ptr(index), st)
    return (vertices, colors, faces, index) if return_index else (vertices, colors, faces)


def _host(a, dtype) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def _write_vertices(f, p: np.ndarray, c: np.ndarray, binary: bool, faces: Optional[int] = None) -> None:
    """Header and vertex body of a PLY (with a face element of `faces` rows when given): one structured array, or the
    reference's ASCII lines (%.6f)."""
    face = "" if faces is None else f"element face {faces}\nproperty list uchar int vertex_indices\n"
    f.write(("ply\nformat {} 1.0\nelement vertex {}\nproperty float x\nproperty float y\nproperty float z\n"
             "property uchar red\nproperty uchar green\nproperty uchar blue\n{}end_header\n"
             ).format("binary_little_endian" if binary else "ascii", p.shape[0], face).encode("ascii"))
    if binary:
        body = np.empty(p.shape[0], dtype=_PLY_DTYPE)
        body["x"], body["y"], body["z"] = p[:, 0], p[:, 1], p[:, 2]
        body["red"], body["green"], body["blue"] = c[:, 0], c[:, 1], c[:, 2]
        body.tofile(f)
    elif p.shape[0]:
        np.savetxt(f, np.concatenate([p.astype(np.float64), c.astype(np.float64)], axis=1), fmt="%.6f %.6f %.6f %d %d %d")


def save_ply(path, points, colors, binary: bool = True) -> int:
    """PLY with the reference's vertex properties (float x y z, uchar red green blue; slam.py:395-412).  binary: one
    structured array written in `binary_little_endian 1.0`; else the reference's ASCII lines (%.6f).  Returns M."""
    p = _host(points, np.float32).reshape(-1, 3)
    c = _host(colors, np.uint8).reshape(-1, 3)
    if p.shape[0] != c.shape[0]:
        raise ValueError(f"{p.shape[0]} points but {c.shape[0]} colours")
    with open(os.fspath(path), "wb") as f:
        _write_vertices(f, p, c, binary)
    return p.shape[0]


def save_ply_mesh(path, vertices, colors, faces, binary: bool = True):
    """PLY with save_ply's vertex properties plus `element face F` / `property list uchar int vertex_indices`.  binary:
    two structured arrays (vertices, then faces) in `binary_little_endian 1.0`; else ASCII lines, for small meshes.
    ValueError when a face index is outside [0, V).  Returns (V, F)."""
    p = _host(vertices, np.float32).reshape(-1, 3)
    c = _host(colors, np.uint8).reshape(-1, 3)
    t = _host(faces, np.int32).reshape(-1, 3)
    if p.shape[0] != c.shape[0]:
        raise ValueError(f"{p.shape[0]} vertices but {c.shape[0]} colours")
    v, f = p.shape[0], t.shape[0]
    if f and (int(t.min()) < 0 or int(t.max()) >= v):
        raise ValueError(f"face indices span [{int(t.min())}, {int(t.max())}], the mesh has {v} vertices")
    with open(os.fspath(path), "wb") as fh:
        _write_vertices(fh, p, c, binary, faces=f)
        if binary:
            tri = np.empty(f, dtype=_PLY_FACE_DTYPE)
            tri["n"], tri["v"] = 3, t
            tri.tofile(fh)
        elif f:
            np.savetxt(fh, t, fmt="3 %d %d %d")
    return v, f


def save_ply_mesh_normals(path, vertices, colors, faces, normals, binary: bool = True):
    """save_ply_mesh with per-vertex normals (normals.vertex_normals): the vertex properties are float x y z nx ny nz,
    uchar red green blue - the order MeshLab, Open3D and CloudCompare write - followed by the face element as
    save_ply_mesh writes it.  binary: two structured arrays in `binary_little_endian 1.0`; else ASCII lines (%.6f), for
    small meshes.  ValueError when the row counts differ or a face index is outside [0, V).  Returns (V, F)."""
    p = _host(vertices, np.float32).reshape(-1, 3)
    c = _host(colors, np.uint8).reshape(-1, 3)
    t = _host(faces, np.int32).reshape(-1, 3)
    n = _host(normals, np.float32).reshape(-1, 3)
    if p.shape[0] != c.shape[0] or p.shape[0] != n.shape[0]:
        raise ValueError(f"{p.shape[0]} vertices but {c.shape[0]} colours and {n.shape[0]} normals")
    v, f = p.shape[0], t.shape[0]
    if f and (int(t.min()) < 0 or int(t.max()) >= v):
        raise ValueError(f"face indices span [{int(t.min())}, {int(t.max())}], the mesh has {v} vertices")
    with open(os.fspath(path), "wb") as fh:
        fh.write(("ply\nformat {} 1.0\nelement vertex {}\nproperty float x\nproperty float y\nproperty float z\n"
                  "property float nx\nproperty float ny\nproperty float nz\n"
                  "property uchar red\nproperty uchar green\nproperty uchar blue\n"
                  "element face {}\nproperty list uchar int vertex_indices\nend_header\n"
                  ).format("binary_little_endian" if binary else "ascii", v, f).encode("ascii"))
        if binary:
            body = np.empty(v, dtype=_PLY_NORMALS_DTYPE)
            for k, name in enumerate("xyz"):
                body[name], body["n" + name] = p[:, k], n[:, k]
            body["red"], body["green"], body["blue"] = c[:, 0], c[:, 1], c[:, 2]
            body.tofile(fh)
            tri = np.empty(f, dtype=_PLY_FACE_DTYPE)
            tri["n"], tri["v"] = 3, t
            tri.tofile(fh)
        else:
            if v:
                np.savetxt(fh, np.concatenate([p.astype(np.float64), n.astype(np.float64), c.astype(np.float64)], axis=1),
                           fmt="%.6f %.6f %.6f %.6f %.6f %.6f %d %d %d")
            if f:
                np.savetxt(fh, t, fmt="3 %d %d %d")
    return v, f


def save_ply_normals(path, points, colors, normals, binary: bool = True) -> int:
    """save_ply with per-point normals (cloud.cloud_normals): the vertex properties are float x y z nx ny nz, uchar red
    green blue, as save_ply_mesh_normals writes them, and there is no face element - what a Poisson reconstruction or a
    surfel viewer reads.  binary: one structured array in `binary_little_endian 1.0`; else ASCII lines (%.6f), for
    small clouds.  ValueError when the row counts differ.  Returns M."""
    p = _host(points, np.float32).reshape(-1, 3)
    c = _host(colors, np.uint8).reshape(-1, 3)
    n = _host(normals, np.float32).reshape(-1, 3)
    if p.shape[0] != c.shape[0] or p.shape[0] != n.shape[0]:
        raise ValueError(f"{p.shape[0]} points but {c.shape[0]} colours and {n.shape[0]} normals")
    m = p.shape[0]
    with open(os.fspath(path), "wb") as fh:
        fh.write(("ply\nformat {} 1.0\nelement vertex {}\nproperty float x\nproperty float y\nproperty float z\n"
                  "property float nx\nproperty float ny\nproperty float nz\n"
                  "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n"
                  ).format("binary_little_endian" if binary else "ascii", m).encode("ascii"))
        if binary:
            body = np.empty(m, dtype=_PLY_NORMALS_DTYPE)
            for k, name in enumerate("xyz"):
                body[name], body["n" + name] = p[:, k], n[:, k]
            body["red"], body["green"], body["blue"] = c[:, 0], c[:, 1], c[:, 2]
            body.tofile(fh)
        elif m:
            np.savetxt(fh, np.concatenate([p.astype(np.float64), n.astype(np.float64), c.astype(np.float64)], axis=1),
                       fmt="%.6f %.6f %.6f %.6f %.6f %.6f %d %d %d")
    return m


def _sim3_rows(poses: np.ndarray) -> np.ndarray:
    """[F,8] (t, q xyzw, s) -> [F,12]: the first three rows of [sR | t], float64, the reference's quaternion formula
    (liegroups/so3.py:174-205, no normalisation)."""
    t, (x, y, z, w), s = poses[:, :3], poses[:, 3:7].T, poses[:, 7]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
    return np.concatenate([s[:, None, None] * R, t[:, :, None]], axis=2).reshape(-1, 12)


def save_trajectory(path, timestamps: Sequence, poses, format: str = "tum") -> int:
    """slam.py:354-381 on [F,8] pose rows.  "tum": `ts tx ty tz qx qy qz qw`; "kitti": the 12 numbers of [sR | t] row by
    row; all %.6f.  Any other format raises ValueError (the reference writes nothing).  Returns the line count."""
    if format not in ("tum", "kitti"):
        raise ValueError(f"unknown trajectory format {format!r}; expected 'tum' or 'kitti'")
    P = _host(poses, np.float64).reshape(-1, 8)
    ts = np.asarray([float(t) for t in timestamps], dtype=np.float64)
    if format == "tum" and ts.shape[0] != P.shape[0]:
        raise ValueError(f"{ts.shape[0]} timestamps but {P.shape[0]} poses")
    rows = np.concatenate([ts[:, None], P[:, :7]], axis=1) if format == "tum" else _sim3_rows(P)
    with open(os.fspath(path), "w") as f:
        for r in rows:
            f.write(" ".join("%.6f" % v for v in r) + "\n")
    return rows.shape[0]
