"""Headless map renderer: colour, depth and index views of the keyframe map, drawn on the device (csrc/render.hip).

The reference shows its map in a desktop GUI (thirdparty/in3d) fed by the `callback` of SLAM.run; an MI355X has no
display.  render_map draws the map as it stands on the device into an image from any pinhole camera:

    candidate(k, n)  <=>  export.collect_map's rule: C[k][n] / N_k > c_conf_threshold (None: no test), world point finite
    camera point     c = R_v^T (p - t_v) / s_v          (inverse of the view pose formed in float64, rounded to fp32)
    kept             <=>  near < c.z < far               (strict)
    pixel            floor(fx * c.x / c.z + cx + 0.5), floor(fy * c.y / c.z + cy + 0.5): integers are pixel centres
    footprint        point_size x point_size pixels around it
    winner           the nearest candidate per pixel, equal depths go to the smaller source index k * N + n

One call queues three launches whatever the number of keyframes, reads nothing back and allocates nothing when `out`
and `workspace` are given; the view pose is read on the device, so a tracked pose can be used as it is and the call
can be captured into a graph.  Two calls give identical bytes.  CPU tensors raise RuntimeError: there is no CPU path.

render_mesh draws a triangle mesh (export.collect_mesh, fusion.extract_surface) the same way: solid surfaces instead of
single points, four launches whatever the mesh size (csrc/raster.hip).
"""
from __future__ import annotations

import math
import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import _ffi
from ._mesh_args import check_shape3, take_workspace
from ._view_args import _outputs, _pinhole, _view_args, _view_pose
from .export import _MapTables, _conf_gate, _map_tables, collect_mesh

__all__ = ["render_map", "render_mesh", "mesh_workspace_bytes", "default_intrinsics", "look_at", "behind", "depth_to_rgb",
           "save_image", "ViewRecorder"]

POINT_SIZES = (1, 3, 5, 7)
CULL = {"none": 0, "back": 1}
SHADING = (None, "headlight", "normals")


def default_intrinsics(size: Sequence[int], fov_deg: float = 60.0):
    """(fx, fy, cx, cy) of a pinhole with square pixels and a horizontal field of view of `fov_deg` for size = (H, W);
    the principal point is the image centre in pixel-centre coordinates."""
    h, w = int(size[0]), int(size[1])
    if h <= 0 or w <= 0:
        raise ValueError(f"size must be positive, got {tuple(size)}")
    if not 0.0 < float(fov_deg) < 180.0:
        raise ValueError(f"fov_deg must lie in (0, 180), got {fov_deg}")
    f = 0.5 * w / math.tan(math.radians(float(fov_deg)) / 2.0)
    return (f, f, (w - 1) / 2.0, (h - 1) / 2.0)


def look_at(eye, target, up=(0.0, -1.0, 0.0)) -> torch.Tensor:
    """[1,8] float32 pose (t, q xyzw, s = 1) of a camera at `eye` whose +z axis points at `target`, +x to the right and
    +y down (the image convention of the projection above), computed on the host in float64.  `up` is the world's up
    direction; the default suits a map whose first camera is upright (y down)."""
    e, t, u = (np.asarray(v, dtype=np.float64).reshape(3) for v in (eye, target, up))
    z = t - e
    if not np.linalg.norm(z) > 0.0:
        raise ValueError("look_at: eye and target coincide")
    z = z / np.linalg.norm(z)
    x = np.cross(z, u)
    if not np.linalg.norm(x) > 1e-12 * max(1.0, np.linalg.norm(u)):
        raise ValueError("look_at: up is parallel to the viewing direction")
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], axis=1)                                      # columns: the camera axes in the world
    # quaternion of a rotation matrix, the branch with the largest pivot; w >= 0
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0.0:
        s = 2.0 * math.sqrt(1.0 + tr)
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    else:
        i = int(np.argmax([R[0, 0], R[1, 1], R[2, 2]]))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * math.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        q = [0.0, 0.0, 0.0, (R[k, j] - R[j, k]) / s]
        q[i], q[j], q[k] = 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s
    q = np.asarray(q)
    if q[3] < 0.0:
        q = -q
    return torch.from_numpy(np.concatenate([e, q, [1.0]])[None]).to(torch.float32)


def behind(T_WC: torch.Tensor, distance: float = 1.0, height: float = 0.25) -> torch.Tensor:
    """Chase camera for a tracked pose: the same orientation, moved `distance` back along the camera's viewing axis and
    `height` up (against its +y axis), unit scale: t' = t + R (0, -height, -distance), q' = q, s' = 1.  Plain tensor
    operations on T_WC's own device: a tracked pose needs no host round trip."""
    T = T_WC.reshape(-1, 8)[:1]
    t, qv, w = T[:, :3], T[:, 3:6], T[:, 6:7]
    v = torch.tensor([[0.0, -float(height), -float(distance)]], dtype=T.dtype, device=T.device)
    u = 2.0 * torch.linalg.cross(qv, v)
    return torch.cat([t + v + w * u + torch.linalg.cross(qv, u), T[:, 3:7], torch.ones_like(w)], dim=1)


def map_tables(keyframes):
    """The device tables render_map builds from `keyframes` on every call (three small host-to-device copies), built once:
    pass the result as `keyframes` to draw the same map again without them, e.g. inside a graph capture, where a copy
    from host memory is not allowed.  Valid while the keyframes' tensors are neither reallocated nor freed; None for an
    empty map."""
    return _map_tables(keyframes)


def workspace_bytes(size: Sequence[int]) -> int:
    """Bytes of the key buffer render_map needs for size = (H, W)."""
    n = int(_ffi.lib().m3_render_ws_bytes(int(size[0]), int(size[1])))
    if n <= 0:
        raise ValueError(f"unsupported view size {tuple(size)} (each side 1 ... 16384)")
    return n


def render_map(keyframes, T_WC, K, size, c_conf_threshold: Optional[float] = 1.5, point_size: int = 1,
               near: float = 1e-3, far: float = math.inf, background=(0, 0, 0), return_index: bool = False, out=None,
               workspace: Optional[torch.Tensor] = None):
    """(rgb uint8 [H,W,3], depth float32 [H,W][, index int64 [H,W]]) of `keyframes` (as collect_map takes them) seen from
    the Sim(3) pose T_WC ([1,8] or [8] float32 DEVICE tensor, read by the kernel) through the pinhole K = (fx, fy, cx,
    cy) (or a 3 x 3 matrix; None: default_intrinsics(size)), size = (H, W).

    depth is the camera-frame z of the winning point (+inf where nothing was drawn), index its source index k * N + n
    (-1 where nothing was drawn).  `keyframes` may also be the result of map_tables(keyframes).  `out`: a tuple of tensors to write into instead of allocating; `workspace`: a uint8
    device tensor of workspace_bytes(size).  An empty map gives the background image."""
    if point_size not in POINT_SIZES:
        raise ValueError(f"point_size must be one of {POINT_SIZES}, got {point_size}")
    hv, wv, (fx, fy, cx, cy), near, far, bg = _view_args(size, K, near, far, background)
    ws_bytes = workspace_bytes((hv, wv))
    m = keyframes if isinstance(keyframes, _MapTables) else _map_tables(keyframes)
    view = _view_pose(T_WC)
    dev = view.device
    if m is not None and m.device != dev:
        raise ValueError(f"T_WC lives on {dev}, the map on {m.device}")
    out = _outputs(out, return_index, hv, wv, dev)
    workspace = take_workspace(workspace, ws_bytes, dev, owner=None)
    use, thr = _conf_gate(c_conf_threshold)
    if m is None:
        tabs, poses, nk, k, n, layout = (None, None, None), None, None, 0, 1, 0
    else:
        tabs, poses, nk, k, n, layout = m.table, m.poses, m.nk, m.k, m.n, m.layout
    _ffi.call("m3_render_map", _ffi.ptr(tabs[0]), _ffi.ptr(tabs[1]), _ffi.ptr(tabs[2]), _ffi.ptr(poses), _ffi.ptr(nk), k, n,
              use, thr, layout, _ffi.ptr(view), fx, fy, cx, cy, hv, wv, near, far, int(point_size), bg[0], bg[1], bg[2],
              _ffi.ptr(workspace), ws_bytes, _ffi.ptr(out[0]), _ffi.ptr(out[1]), _ffi.ptr(out[2]) if return_index else None,
              _ffi.stream_ptr())
    return out


def mesh_workspace_bytes(n_vertices: int, size: Sequence[int]) -> int:
    """Bytes of the workspace render_mesh needs for a mesh of n_vertices and size = (H, W): a 16-byte record per vertex and
    the dense key buffer of H * W * 8 bytes."""
    n = int(_ffi.lib().m3_raster_ws_bytes(int(n_vertices), int(size[0]), int(size[1])))
    if n <= 0:
        raise ValueError(f"unsupported view size {tuple(size)} (each side 1 ... 16384) or vertex count {n_vertices} "
                         "(at most 2^31 - 1)")
    return n


def render_mesh(vertices, colors=None, faces=None, T_WC=None, K=None, size=None, near: float = 1e-3, far: float = math.inf,
                cull: str = "none", background=(0, 0, 0), return_index: bool = False, out=None,
                workspace: Optional[torch.Tensor] = None, shading: Optional[str] = None, normals: Optional[torch.Tensor] = None,
                shade_kw=None):
    """(rgb uint8 [H,W,3], depth float32 [H,W][, index int64 [H,W]]) of a triangle mesh - vertices float32 [V,3] in world
    coordinates, colors uint8 [V,3], faces int32 [F,3], as export.collect_mesh, SLAM.mesh, fusion.extract_surface and
    SLAM.fused_mesh return them - seen from the Sim(3) pose T_WC through the pinhole K, size = (H, W), all three as for
    render_map.  The tuple those functions return may also be passed whole: render_mesh(mesh, T_WC, K, size).

    A pixel whose centre a face covers (integer arithmetic on a grid of 256 steps per pixel, top-left rule: faces that
    share an edge neither overlap nor leave a crack) gets the perspective-correct depth and the smoothly blended vertex
    colours of the nearest such face, equal depths going to the smaller face index.  depth is +inf and index (the face
    index) -1 where nothing was drawn.  cull "back" drops the faces that are clockwise on the screen (y down), which
    keeps collect_mesh's faces seen from the side of their keyframe; "none" draws both windings.  Faces with an index
    outside [0, V) are skipped.  `out` and `workspace` (mesh_workspace_bytes(V, size) bytes) as for render_map.

    Known limitation: there is no clipping.  A face with a vertex at or behind `near`, at or beyond `far`, or more than
    16384 pixels from the image origin is dropped whole, so a surface that passes close by the camera gets holes.
    Smooth shading only; V and F at most 2^31 - 1.

    shading None draws the vertex colours as they are.  "headlight" draws them lit by a point light at the eye of T_WC
    and "normals" draws the world-space vertex normals as colours: normals.shade_vertices(vertices, normals, colors,
    T_WC, **shade_kw) into a temporary, which is rasterised in the place of `colors` (shade_kw: shade_vertices' light,
    ambient, two_sided and albedo; colors=None there draws the constant albedo, shape without the photographs).
    `normals` (float32 [V,3]) are normals.vertex_normals(vertices, faces) unless given: 3 + 1 + 4 launches, nothing
    read back, and the temporaries are the only allocations."""
    if isinstance(vertices, (tuple, list)):
        if colors is not None:                                              # render_mesh(mesh, T_WC, K, size)
            T_WC, K, size = colors, (faces if faces is not None else K), (T_WC if T_WC is not None else size)
        if len(vertices) < 3:
            raise ValueError("a mesh is (vertices, colors, faces[, index])")
        vertices, colors, faces = vertices[:3]
    if size is None or T_WC is None:
        raise ValueError("render_mesh needs T_WC and size")
    hv, wv, (fx, fy, cx, cy), near, far, bg = _view_args(size, K, near, far, background)
    if cull not in CULL:
        raise ValueError(f"cull must be one of {tuple(CULL)}, got {cull!r}")
    if shading not in SHADING:
        raise ValueError(f"shading must be one of {SHADING}, got {shading!r}")
    if shading is None and (normals is not None or shade_kw):
        raise ValueError("normals and shade_kw are for shading='headlight' or 'normals'")
    if not set(shade_kw or {}) <= {"light", "ambient", "two_sided", "albedo", "colors"}:
        raise ValueError(f"shade_kw holds shade_vertices' light, ambient, two_sided, albedo and colors, got {sorted(shade_kw)}")
    for t, dt, name in ((vertices, torch.float32, "vertices"), (colors, torch.uint8, "colors"), (faces, torch.int32, "faces")):
        check_shape3(t, dt, name)
    if colors.shape[0] != vertices.shape[0]:
        raise ValueError(f"vertices has {vertices.shape[0]} rows, colors {colors.shape[0]}")
    v, f = int(vertices.shape[0]), int(faces.shape[0])
    view = _view_pose(T_WC)
    dev = view.device
    vertices, colors, faces = (_ffi.check(t, t.dtype, name) for t, name in ((vertices, "vertices"), (colors, "colors"), (faces, "faces")))
    if any(t.device != dev for t in (vertices, colors, faces)):
        raise ValueError(f"T_WC lives on {dev}, the mesh on {vertices.device}")
    ws_bytes = mesh_workspace_bytes(v, (hv, wv))
    out = _outputs(out, return_index, hv, wv, dev)
    if shading is not None:
        from . import normals as _normals                                    # normals imports export, as this module does
        if normals is None:
            normals = _normals.vertex_normals(vertices, faces)
        kw = dict(colors=colors, T_WC=view, mode="normals" if shading == "normals" else "lambert")
        kw.update(shade_kw or {})
        colors = _normals.shade_vertices(vertices, normals, **kw)
    workspace = take_workspace(workspace, ws_bytes, dev, owner=None)
    _ffi.call("m3_raster_mesh", _ffi.ptr(vertices) if v else None, _ffi.ptr(colors) if v else None, _ffi.ptr(faces) if f else None,
              v, f, _ffi.ptr(view), fx, fy, cx, cy, hv, wv, near, far, CULL[cull], bg[0], bg[1], bg[2], _ffi.ptr(workspace),
              ws_bytes, _ffi.ptr(out[0]), _ffi.ptr(out[1]), _ffi.ptr(out[2]) if return_index else None, _ffi.stream_ptr())
    return out


def depth_to_rgb(depth: torch.Tensor, near: Optional[float] = None, far: Optional[float] = None) -> torch.Tensor:
    """Grey image uint8 [H,W,3] of a rendered depth: near -> white, far -> dark grey (32), nothing drawn (+inf) -> black.
    near / far default to the smallest / largest finite depth."""
    d = depth.to(torch.float32)
    ok = torch.isfinite(d)
    lo = torch.where(ok, d, torch.full_like(d, math.inf)).min() if near is None else torch.tensor(float(near), device=d.device)
    hi = torch.where(ok, d, torch.full_like(d, -math.inf)).max() if far is None else torch.tensor(float(far), device=d.device)
    t = ((d - lo) / (hi - lo).clamp_min(1e-30)).clamp(0.0, 1.0)
    g = torch.where(ok, 255.0 - 223.0 * torch.nan_to_num(t, nan=0.0, posinf=1.0), torch.zeros_like(d)).floor().to(torch.uint8)
    return g[..., None].expand(*g.shape, 3).contiguous()


def save_image(path, rgb) -> None:
    """PNG of a uint8 [H,W,3] image (one device-to-host copy)."""
    from PIL import Image
    a = rgb.detach().cpu().numpy() if isinstance(rgb, torch.Tensor) else np.asarray(rgb)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"expected a uint8 [H,W,3] image, got {a.dtype} {a.shape}")
    Image.fromarray(np.ascontiguousarray(a), "RGB").save(os.fspath(path), format="PNG")


def scaled_intrinsics(K, from_size: Sequence[int], to_size: Sequence[int]):
    """(fx, fy, cx, cy) of `K` (given for an image of from_size = (H, W)) moved to to_size, pixel-centre coordinates."""
    fx, fy, cx, cy = _pinhole(K, from_size)
    sy, sx = to_size[0] / from_size[0], to_size[1] / from_size[1]
    return fx * sx, fy * sy, (cx + 0.5) * sx - 0.5, (cy + 0.5) * sy - 0.5


def _frame_size(img: torch.Tensor):
    return (int(img.shape[1]), int(img.shape[2])) if img.dtype != torch.uint8 else (int(img.shape[0]), int(img.shape[1]))


class ViewRecorder:
    """callback(frame, keyframes) for SLAM.run / run_dataset: renders the map after every `every`-th frame and writes
    directory/view_%06d.png (numbered by frame_id).

    camera: "follow" (behind(frame.T_WC, follow_distance, follow_height)), "frame" (the frame's own pose) or a fixed
    [1,8] pose.  K None: the frame's intrinsics moved to `size`, else default_intrinsics(size).  The output tensors
    and the workspace are allocated once; per frame the host reads back the finished image and nothing else.

    surface "mesh" draws export.collect_mesh(keyframes, **mesh_kw) with render_mesh instead of the points with render_map
    (render_kwargs are then render_mesh's; shading="headlight" records lit views).  The mesh is collected again for every
    recorded frame, which costs collect_mesh's one host read of the vertex and face counts, and the workspace grows with
    the vertex count."""

    def __init__(self, directory, every: int = 1, camera="follow", size: Sequence[int] = (480, 640), K=None,
                 follow_distance: float = 1.0, follow_height: float = 0.25, surface: str = "points", mesh_kw=None,
                 **render_kwargs) -> None:
        if int(every) < 1:
            raise ValueError(f"every must be >= 1, got {every}")
        if surface == "fused":
            raise ValueError("surface 'fused' is too costly per frame (a TSDF fusion of the whole map for every recorded "
                             "frame): record 'points' or 'mesh', and draw the fused mesh once with SLAM.render_view")
        if surface not in ("points", "mesh"):
            raise ValueError(f"surface must be 'points' or 'mesh', got {surface!r}")
        if mesh_kw and surface != "mesh":
            raise ValueError("mesh_kw is for surface='mesh'")
        if isinstance(camera, str) and camera not in ("follow", "frame"):
            raise ValueError(f"camera must be 'follow', 'frame' or a pose, got {camera!r}")
        if "return_index" in render_kwargs or "out" in render_kwargs or "workspace" in render_kwargs:
            raise ValueError("the recorder owns its outputs: return_index / out / workspace cannot be passed")
        if surface == "points" and any(render_kwargs.get(k) is not None for k in ("shading", "normals", "shade_kw")):
            raise ValueError("shading is for surface='mesh': points carry no normals")
        self.directory = os.fspath(directory)
        os.makedirs(self.directory, exist_ok=True)
        self.every, self.camera, self.size, self.K = int(every), camera, (int(size[0]), int(size[1])), K
        self.follow = (float(follow_distance), float(follow_height))
        self.render_kwargs = render_kwargs
        self.surface, self.mesh_kw = surface, dict(mesh_kw or {})
        self.calls = 0
        self.paths: list[str] = []
        self.last_pose: Optional[torch.Tensor] = None
        self._out = self._ws = None

    def view_pose(self, frame) -> torch.Tensor:
        if isinstance(self.camera, str):
            return behind(frame.T_WC, *self.follow) if self.camera == "follow" else frame.T_WC.reshape(1, 8)
        return torch.as_tensor(self.camera, dtype=torch.float32).reshape(1, 8).to(frame.T_WC.device)

    def intrinsics(self, frame):
        if self.K is not None:
            return _pinhole(self.K, self.size)
        if getattr(frame, "K", None) is not None:
            return scaled_intrinsics(frame.K, _frame_size(frame.img), self.size)
        return default_intrinsics(self.size)

    def __call__(self, frame, keyframes) -> Optional[str]:
        self.calls += 1
        if (self.calls - 1) % self.every:
            return None
        pose = self.view_pose(frame).to(torch.float32).contiguous()
        if self._out is None:
            dev = pose.device
            self._out = (torch.empty((*self.size, 3), dtype=torch.uint8, device=dev),
                         torch.empty(self.size, dtype=torch.float32, device=dev))
            self._ws = torch.empty((workspace_bytes(self.size),), dtype=torch.uint8, device=dev)
        if self.surface == "mesh":
            mesh = collect_mesh(keyframes, **self.mesh_kw)[:3]
            need = mesh_workspace_bytes(mesh[0].shape[0], self.size)
            if self._ws.numel() < need:
                self._ws = torch.empty((need,), dtype=torch.uint8, device=pose.device)
            rgb, _ = render_mesh(*mesh, pose, self.intrinsics(frame), self.size, out=self._out, workspace=self._ws,
                                 **self.render_kwargs)
        else:
            rgb, _ = render_map(keyframes, pose, self.intrinsics(frame), self.size, out=self._out, workspace=self._ws,
                                **self.render_kwargs)
        path = os.path.join(self.directory, "view_%06d.png" % int(frame.frame_id))
        save_image(path, rgb)
        self.last_pose = pose.clone()
        self.paths.append(path)
        return path
