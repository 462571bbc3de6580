"""Connected components of a triangle mesh on the device, and the clean-up that drops small fragments
(csrc/mesh_components.hip).

collect_mesh leaves the patches between depth discontinuities, extract_surface the few voxels that gathered weight from
one noisy keyframe: small islands of triangles floating off the surface.  mesh_components labels which triangles hang
together, filter_components keeps the large components.

    connectivity       by row of the vertex arrays, never by position: two vertices are connected when a face names both
    label[v]           the smallest row in the component of v; a vertex no face names is its own component with 0 faces
    faces_of[c]        the faces whose first row lies in component c;  largest = the maximum;  the winner attains it, a
                       tie going to the smaller label
    kept component     faces_of >= max(1, min_faces), and min_fraction == 0 or faces_of >= min_fraction * largest (one
                       float64 multiply and compare, min_fraction rounded to fp32 first), and not largest_only or it is
                       the winner
    outputs            the vertices and faces of kept components in their input order, faces rewritten to the new rows

The exact rule is in include/m3slam.h.  Everything is integer work whose result does not depend on the execution order,
and output rows come from an ordered compaction: two calls give identical bytes.  Component area and any other float
criterion are left out (a float sum over atomics is not reproducible).  A call queues 11 launches whatever the mesh holds
(6 to label, 3 to count, 2 to scatter) and reads one 32-byte header back between the count and the scatter.  CPU tensors
raise RuntimeError: there is no CPU path.
"""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from . import _ffi
from ._mesh_args import check_faces, check_mesh, empty_mesh_with_index, raise_invalid_faces, take_workspace, unpack_mesh

__all__ = ["mesh_components", "filter_components", "ComponentsInfo", "workspace_bytes"]

ComponentsInfo = namedtuple("ComponentsInfo", ["components", "largest", "winner"])
ComponentsInfo.__doc__ = ("components: the components with at least one face; largest: the faces of the largest one; winner: its "
                          "label, the smaller label on a tie (-1 when the mesh has no face).")

MAX_ROWS = 2 ** 31 - 1                                                  # include/m3slam.h
_HDR_WORDS = 8                                                          # V2, F2, -, -, components, largest, winner, invalid


def workspace_bytes(n_vertices: int, n_faces: int) -> int:
    """Bytes of the workspace mesh_components / filter_components need for a mesh of n_vertices and n_faces."""
    b = int(_ffi.lib().m3_mesh_components_ws_bytes(int(n_vertices), int(n_faces)))
    if b <= 0:
        raise ValueError(f"unsupported mesh of {n_vertices} vertices and {n_faces} faces (each 0 ... 2^31 - 1)")
    return b


def _label(faces: torch.Tensor, v: int, workspace: Optional[torch.Tensor], labels, faces_of) -> torch.Tensor:
    """Queue the labelling of `faces` over v vertex rows; returns the workspace."""
    f = int(faces.shape[0])
    ws_bytes = workspace_bytes(v, f)
    workspace = take_workspace(workspace, ws_bytes, faces.device)
    _ffi.call("m3_mesh_components_label", _ffi.ptr(faces) if f else None, v, f, _ffi.ptr(workspace), ws_bytes, _ffi.ptr(labels),
              _ffi.ptr(faces_of), _ffi.stream_ptr())
    return workspace


def mesh_components(faces, n_vertices: int, workspace: Optional[torch.Tensor] = None):
    """(labels int32 [V], faces_of int32 [V], info) of the mesh `faces` (int32 [F,3], a device tensor) over V = n_vertices
    rows: labels[v] is the smallest row in the component of v, faces_of[v] the number of faces of that component (the
    faces whose first row lies in it), info a ComponentsInfo.  A vertex named by no face keeps its own row as its label,
    with 0 faces.  A face that names a row twice connects its rows and counts.  One host read (the header, 32 bytes).
    workspace: a 16-byte aligned uint8 device tensor of workspace_bytes(V, F).  ValueError when a face names a row outside
    [0, V); RuntimeError for CPU tensors."""
    v = int(n_vertices)
    if v != n_vertices or v < 0 or v > MAX_ROWS:
        raise ValueError(f"n_vertices must be an integer in 0 ... 2^31 - 1, got {n_vertices}")
    faces = check_faces(faces)
    dev = faces.device
    labels = torch.empty((v,), dtype=torch.int32, device=dev)
    faces_of = torch.empty((v,), dtype=torch.int32, device=dev)
    ws = _label(faces, v, workspace, labels, faces_of)
    hdr = ws[:4 * _HDR_WORDS].view(torch.int32).tolist()                  # the one synchronisation
    raise_invalid_faces(hdr[7], v)
    return labels, faces_of, ComponentsInfo(hdr[4], hdr[5], hdr[6])


def filter_components(vertices, colors=None, faces=None, min_faces: int = 1, min_fraction: float = 0.0,
                      largest_only: bool = False, return_index: bool = False, workspace: Optional[torch.Tensor] = None):
    """(vertices float32 [V2,3], colors uint8 [V2,3], faces int32 [F2,3][, vertex_rows int64 [V2], face_rows int64 [F2]]) of
    the kept components of a mesh, as device tensors.  The mesh is passed unpacked or as the tuple export.collect_mesh,
    fusion.extract_surface, SLAM.mesh and SLAM.fused_mesh return: filter_components(mesh, min_faces=50).

    A component is kept when it has at least max(1, min_faces) faces, at least min_fraction (0 ... 1, rounded to fp32; 0:
    no test) of the faces of the largest component, and - largest_only - is the largest one (a tie goes to the component
    with the smaller first row).  Kept vertices and faces come out in their input order, faces rewritten to the new rows;
    a vertex no face names is dropped by every filter.  return_index adds the input row of every output vertex and face.
    An empty mesh in, or a filter that keeps nothing, gives the empty mesh.  workspace as for mesh_components.  ValueError
    when a face names a row outside [0, V), for a min_fraction outside [0, 1] or a min_faces that is no integer;
    RuntimeError for CPU tensors."""
    vertices, colors, faces = unpack_mesh(vertices, colors, faces)
    if isinstance(min_faces, bool) or int(min_faces) != min_faces or abs(int(min_faces)) > MAX_ROWS:
        raise ValueError(f"min_faces must be an integer, got {min_faces}")
    fraction = float(np.float32(min_fraction))
    if not 0.0 <= fraction <= 1.0 or math.isnan(fraction):
        raise ValueError(f"min_fraction must lie in [0, 1], got {min_fraction}")
    vertices, colors, faces = check_mesh(vertices, colors, faces, rows_first=True)
    dev = faces.device
    v, f = int(vertices.shape[0]), int(faces.shape[0])
    if v == 0 and f == 0:
        return empty_mesh_with_index(dev, return_index)
    ws = _label(faces, v, workspace, None, None)
    st = _ffi.stream_ptr()
    _ffi.call("m3_mesh_components_count", _ffi.ptr(ws), v, f, _ffi.ptr(faces) if f else None, int(min_faces), fraction,
              1 if largest_only else 0, st)
    hdr = ws[:4 * _HDR_WORDS].view(torch.int32).tolist()                  # the one synchronisation: V2, F2 and the label words
    raise_invalid_faces(hdr[7], v)
    v2, f2 = hdr[0], hdr[1]
    if f2 == 0:
        return empty_mesh_with_index(dev, return_index)
    out_v = torch.empty((v2, 3), dtype=torch.float32, device=dev)
    out_c = torch.empty((v2, 3), dtype=torch.uint8, device=dev)
    out_f = torch.empty((f2, 3), dtype=torch.int32, device=dev)
    rows_v = torch.empty((v2,), dtype=torch.int64, device=dev) if return_index else None
    rows_f = torch.empty((f2,), dtype=torch.int64, device=dev) if return_index else None
    _ffi.call("m3_mesh_components_scatter", _ffi.ptr(vertices), _ffi.ptr(colors), _ffi.ptr(faces), v, f, _ffi.ptr(ws), v2, f2,
              _ffi.ptr(out_v), _ffi.ptr(out_c), _ffi.ptr(out_f), _ffi.ptr(rows_v), _ffi.ptr(rows_f), st)
    return (out_v, out_c, out_f, rows_v, rows_f) if return_index else (out_v, out_c, out_f)

