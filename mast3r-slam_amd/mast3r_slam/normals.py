"""Per-vertex normals of a triangle mesh on the device, and vertex colours lit with them (csrc/mesh_normals.hip,
DESIGN.md section 7l).

The meshes of export.collect_mesh and fusion.extract_surface carry positions and photographed colours.  vertex_normals
adds what a viewer, a PLY reader or a surface reconstruction wants next; shade_vertices turns the normals into lit
vertex colours, which render.render_mesh draws like any others (render_mesh(..., shading="headlight") does both).

    face normal        n = (b - a) x (c - a) in fp32; a face with an index outside [0, V), or with |n|^2 not finite or
                       below 2^-80 (a repeated index, no area, a NaN or infinite vertex) contributes nothing
    contribution       the unit normal n / |n|, every component scaled by 2^24 and rounded to an integer: unit face
                       normals with equal weights, Open3D's rule
    vertex normal      the int64 sum of its faces' contributions, divided by its length in float64 and rounded to fp32;
                       (0, 0, 0) when the sum is zero (no face, only degenerate faces, exact cancellation)

The exact rule is in include/m3slam.h.  The sum is integer work whose result does not depend on the execution order:
two calls give identical bytes, and so do two orders of the faces.  A call queues three operations whatever the mesh
holds, reads nothing back and can be captured into a graph.  CPU tensors raise RuntimeError: there is no CPU path.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _ffi
from ._mesh_args import check_rows3 as _rows3, take_workspace, unpack_mesh, whole_or_unpacked_error

__all__ = ["vertex_normals", "shade_vertices", "workspace_bytes"]

MODES = {"lambert": 0, "normals": 1}


def workspace_bytes(n_vertices: int) -> int:
    """Bytes of the workspace vertex_normals needs for a mesh of n_vertices: three int64 sums per vertex."""
    b = int(_ffi.lib().m3_mesh_normals_ws_bytes(int(n_vertices)))
    if b <= 0:
        raise ValueError(f"unsupported mesh of {n_vertices} vertices (0 ... 2^31 - 1)")
    return b


def _out(out, dtype, v: int, dev, name: str) -> torch.Tensor:
    if out is None:
        return torch.empty((v, 3), dtype=dtype, device=dev)
    if _ffi.check(out, dtype, name, (v, 3)).data_ptr() != out.data_ptr():
        raise ValueError(f"{name} must be contiguous")
    if out.device != dev:
        raise ValueError(f"the mesh lives on {dev}, {name} on {out.device}")
    return out


def vertex_normals(vertices, faces=None, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """normals float32 [V,3] of a mesh - vertices float32 [V,3], faces int32 [F,3], device tensors - by the rule above:
    unit length, or (0, 0, 0) for a vertex without a face of non-zero area.  The tuple export.collect_mesh, SLAM.mesh,
    fusion.extract_surface, SLAM.fused_mesh or components.filter_components return may be passed whole,
    vertex_normals(mesh), or unpacked, vertex_normals(*mesh): a uint8 tensor in the place of `faces` is taken as the
    colours and the faces are looked for behind it.

    The normal of a face (a, b, c) is (b - a) x (c - a): collect_mesh's faces are counter-clockwise seen from their
    keyframe, so their normals face that camera.  Faces with an index outside [0, V) contribute nothing.  `out`: a
    float32 [V,3] device tensor to write into; `workspace`: a 16-byte aligned uint8 device tensor of workspace_bytes(V),
    whose contents are ignored.  F = 0 gives zeros, V = 0 a [0,3] tensor.  RuntimeError for CPU tensors."""
    if isinstance(vertices, (tuple, list)):
        vertices, _, faces = unpack_mesh(vertices, None, faces)
    elif isinstance(faces, torch.Tensor) and faces.dtype == torch.uint8:    # vertex_normals(*mesh): colors, then faces
        if not isinstance(out, torch.Tensor) or out.dtype != torch.int32:
            raise whole_or_unpacked_error()
        faces, out = out, None
        if isinstance(workspace, torch.Tensor) and workspace.dtype == torch.int64:         # the index of a 4-tuple
            workspace = None
    vertices, faces = _rows3((vertices, torch.float32, "vertices"), (faces, torch.int32, "faces"))
    dev = vertices.device
    if faces.device != dev:
        raise ValueError(f"vertices live on {dev}, faces on {faces.device}")
    v, f = int(vertices.shape[0]), int(faces.shape[0])
    ws_bytes = workspace_bytes(v)
    out = _out(out, torch.float32, v, dev, "out")
    workspace = take_workspace(workspace, ws_bytes, dev)
    _ffi.call("m3_mesh_normals", _ffi.ptr(vertices) if v else None, _ffi.ptr(faces) if f else None, v, f, _ffi.ptr(workspace),
              ws_bytes, _ffi.ptr(out) if v else None, _ffi.stream_ptr())
    return out


def _shade_args(T_WC, light, ambient, two_sided, mode, albedo):
    """The scalar arguments of m3_mesh_shade, checked: (light, (lx, ly, lz), ambient, two_sided, mode, albedo)."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {tuple(MODES)}, got {mode!r}")
    ambient = float(np.float32(ambient))
    if not 0.0 <= ambient <= 1.0 or math.isnan(ambient):
        raise ValueError(f"ambient must lie in [0, 1], got {ambient}")
    rgb = tuple(int(c) for c in albedo)
    if len(rgb) != 3 or any(c < 0 or c > 255 for c in rgb):
        raise ValueError(f"albedo must be three values in 0 ... 255, got {albedo}")
    direction = (0.0, 0.0, 0.0)
    if isinstance(light, str):
        if light != "headlight":
            raise ValueError(f"light must be 'headlight' or a 3-vector, got {light!r}")
        if T_WC is None and mode == "lambert":
            raise ValueError("light='headlight' needs the view pose T_WC")
        kind = 0
    else:
        if isinstance(light, torch.Tensor):
            light = light.detach().cpu().tolist()
        d = np.asarray(light, dtype=np.float32).reshape(-1)
        if d.shape != (3,) or not np.isfinite(d).all() or not d.any():
            raise ValueError(f"light must be 'headlight' or a finite, non-zero 3-vector, got {light}")
        kind, direction = 1, tuple(float(x) for x in d)
    return kind, direction, ambient, 1 if two_sided else 0, MODES[mode], rgb


def shade_vertices(vertices, normals, colors=None, T_WC=None, light="headlight", ambient: float = 0.25,
                   two_sided: bool = True, mode: str = "lambert", albedo=(200, 200, 200), out: Optional[torch.Tensor] = None):
    """Lit colours uint8 [V,3] of the vertices of a mesh, for render.render_mesh to draw in the place of `colors`: one
    launch, fp32, nothing read back.

    mode "lambert": colour * (ambient + (1 - ambient) * d), rounded to the nearest level, with d the cosine between the
    normal and the direction to the light, 0 on the far side of the surface; two_sided takes |cosine| instead, which
    suits a mesh whose winding is not known (the fused surface).  light "headlight": a point light at the eye, the
    translation of the view pose T_WC ([1,8] or [8] float32 device tensor, read by the kernel: a replayed graph follows a
    pose rewritten in place); or a 3-vector: the constant world direction from the surface towards the light.  colors
    None: the constant `albedo`.  A vertex whose normal is zero gets the ambient term alone.
    mode "normals": the world-space normal as a colour, (n * 0.5 + 0.5) * 255 rounded; a zero normal gives 128.

    The defaults - a quarter of ambient light, two-sided, a light grey albedo - are this project's choice, not a
    convention taken from elsewhere.  The exact operation order is in include/m3slam.h.  `out`: a uint8 [V,3] device
    tensor to write into.  ValueError for an ambient outside [0, 1], an unknown mode or light, or a zero or non-finite
    light direction; RuntimeError for CPU tensors."""
    kind, (lx, ly, lz), ambient, two, m, rgb = _shade_args(T_WC, light, ambient, two_sided, mode, albedo)
    named = [(vertices, torch.float32, "vertices"), (normals, torch.float32, "normals")]
    if colors is not None:
        named.append((colors, torch.uint8, "colors"))
    rows = _rows3(*named)
    v = int(rows[0].shape[0])
    if any(t.shape[0] != v for t in rows):
        raise ValueError(f"vertices has {v} rows, normals {rows[1].shape[0]}" + (f", colors {rows[2].shape[0]}" if colors is not None else ""))
    vertices, normals, colors = rows[0], rows[1], (rows[2] if colors is not None else None)
    dev = vertices.device
    view = None
    if kind == 0 and m == 0:
        view = _ffi.check(T_WC, torch.float32, "T_WC").reshape(-1)
        if view.numel() != 8:
            raise ValueError(f"T_WC must have 8 elements (t, q xyzw, s), got {tuple(T_WC.shape)}")
    if any(t is not None and t.device != dev for t in (normals, colors, view)):
        raise ValueError(f"vertices live on {dev}; normals, colors and T_WC must live there too")
    out = _out(out, torch.uint8, v, dev, "out")
    _ffi.call("m3_mesh_shade", _ffi.ptr(vertices) if v else None, _ffi.ptr(normals) if v else None, _ffi.ptr(colors) if v else None,
              v, _ffi.ptr(view), kind, lx, ly, lz, ambient, two, m, rgb[0], rgb[1], rgb[2], _ffi.ptr(out) if v else None,
              _ffi.stream_ptr())
    return out
