"""Mesh simplification by vertex clustering on the device (csrc/mesh_simplify.hip).

collect_mesh has one vertex per pixel of every keyframe and extract_surface one per surface cell of the voxel grid, and
overlapping keyframes cover the same surface again and again.  simplify_mesh returns a smaller mesh of the same surface
at a resolution the caller chooses: Open3D's simplify_vertex_clustering with the average made exact.

    cell of a vertex   per axis floor((double)x / voxel), voxel_size rounded to fp32 once; a vertex with a coordinate
                       that is not finite or a cell at or beyond +-2^20 is out of range: it joins no cluster, is counted
                       and is no error
    cluster            the vertices of one cell; its leader is its smallest input row; clusters come out in the order of
                       their leaders, so by first appearance; a cluster of one keeps its vertex's bits and colour, a
                       larger one gets the mean position (offsets in the cell quantised to 2^-24 of it, summed as
                       integers, finished in float64) and the rounded integer mean colour
    faces              mapped to cluster rows; dropped when a row is out of range or two of the three clusters are the
                       same; of the faces over the same clusters with the same winding the smallest input row is kept;
                       kept faces come out in input order, rotated so their smallest row comes first

The exact rule is in include/m3slam.h.  Everything is integer work whose result does not depend on the execution order,
and output rows come from an ordered compaction: two calls give identical bytes.  Every cluster is output, whether or
not a kept face names it (Open3D does the same): filter_components drops the vertices no face names.  Quadric placement
and any error-driven decimation, a target face count, normal-aware clustering and carrying normals through (recompute
them with vertex_normals) are left out.  A call queues 8 launches whatever the mesh holds (6 to count, 2 to scatter) and
reads one 16-byte header back in between.  CPU tensors raise RuntimeError: there is no CPU path.
"""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from . import _ffi
from ._mesh_args import check_mesh, empty_mesh_with_index, raise_invalid_faces, take_workspace, unpack_mesh

__all__ = ["simplify_mesh", "simplify_counts", "SimplifyInfo", "workspace_bytes"]

SimplifyInfo = namedtuple("SimplifyInfo", ["vertices", "faces", "out_of_range"])
SimplifyInfo.__doc__ = ("vertices, faces: the rows of the simplified mesh; out_of_range: the input vertices that joined no "
                        "cluster (a coordinate that is not finite, or a cell at or beyond +-2^20).")

MAX_ROWS = 2 ** 31 - 1                                                  # include/m3slam.h
_HDR_WORDS = 4                                                          # V2, F2, out of range, invalid


def workspace_bytes(n_vertices: int, n_faces: int) -> int:
    """Bytes of the workspace simplify_mesh needs for a mesh of n_vertices and n_faces."""
    b = int(_ffi.lib().m3_mesh_simplify_ws_bytes(int(n_vertices), int(n_faces)))
    if b <= 0:
        raise ValueError(f"unsupported mesh of {n_vertices} vertices and {n_faces} faces (each 0 ... 2^31 - 1)")
    return b


def _voxel(voxel_size) -> float:
    if voxel_size is None:
        raise ValueError("voxel_size is required: the edge of a cluster's cell, in the units of the vertices")
    with np.errstate(over="ignore"):
        voxel = float(np.float32(voxel_size))
    if not (voxel > 0.0 and math.isfinite(voxel)):
        raise ValueError(f"voxel_size must be finite and > 0 (as fp32), got {voxel_size}")
    return voxel


def _mesh(vertices, colors, faces):
    """The three arrays of a mesh passed whole or unpacked, checked: device tensors of the right dtype and shape."""
    return check_mesh(*unpack_mesh(vertices, colors, faces))


def _count(vertices, colors, faces, voxel: float, workspace: Optional[torch.Tensor]):
    """Queue the count stage and read the header: (workspace, V2, F2, out_of_range)."""
    v, f = int(vertices.shape[0]), int(faces.shape[0])
    ws_bytes = workspace_bytes(v, f)
    workspace = take_workspace(workspace, ws_bytes, faces.device)
    _ffi.call("m3_mesh_simplify_count", _ffi.ptr(vertices) if v else None, _ffi.ptr(colors) if v else None,
              _ffi.ptr(faces) if f else None, v, f, voxel, _ffi.ptr(workspace), ws_bytes, _ffi.stream_ptr())
    hdr = workspace[:4 * _HDR_WORDS].view(torch.int32).tolist()          # the one synchronisation
    raise_invalid_faces(hdr[3], v)
    return workspace, hdr[0], hdr[1], hdr[2]


def simplify_counts(vertices, colors=None, faces=None, voxel_size=None, workspace: Optional[torch.Tensor] = None) -> SimplifyInfo:
    """SimplifyInfo(vertices, faces, out_of_range) of simplify_mesh with the same arguments, without building the mesh:
    the count stage and its one host read.  For choosing a voxel_size, and for the number of out-of-range vertices."""
    voxel = _voxel(voxel_size)
    vertices, colors, faces = _mesh(vertices, colors, faces)
    if vertices.shape[0] == 0 and faces.shape[0] == 0:
        return SimplifyInfo(0, 0, 0)
    return SimplifyInfo(*_count(vertices, colors, faces, voxel, workspace)[1:])


def simplify_mesh(vertices, colors=None, faces=None, voxel_size=None, return_index: bool = False,
                  workspace: Optional[torch.Tensor] = None):
    """(vertices float32 [V2,3], colors uint8 [V2,3], faces int32 [F2,3][, cluster_of int64 [V], face_rows int64 [F2]]) of
    the mesh clustered on a grid of voxel_size, as device tensors.  The mesh is passed unpacked or as the tuple
    export.collect_mesh, fusion.extract_surface, SLAM.mesh, SLAM.fused_mesh and filter_components return:
    simplify_mesh(slam.mesh(), voxel_size=0.01).

    One output vertex per occupied cell, in the order in which the cells first appear in the input: a cell with one
    vertex keeps it bit for bit (a voxel_size finer than the mesh returns the vertex and colour arrays unchanged), a cell
    with more gets their mean position and rounded mean colour.  A face is dropped when two of its rows fall into one
    cell or one of them is out of range; of the faces over the same three cells with the same winding the first is kept;
    kept faces come out in input order, each rotated so that its smallest row comes first.  A vertex with a coordinate
    that is not finite, or more than 2^20 cells from the origin, joins no cluster (simplify_counts reports how many).
    Every cluster is output, whether or not a kept face names it, as Open3D does: filter_components drops the vertices
    no face names.  Normals are not carried through: call vertex_normals on the result.

    return_index adds cluster_of (the output row of every input vertex, -1 when out of range) and face_rows (the input
    row of every kept face).  An empty mesh in gives the empty mesh.  workspace: a 16-byte aligned uint8 device tensor of
    workspace_bytes(V, F).  ValueError when voxel_size is missing, not finite or <= 0 and when a face names a row outside
    [0, V); RuntimeError for CPU tensors."""
    voxel = _voxel(voxel_size)
    vertices, colors, faces = _mesh(vertices, colors, faces)
    dev = faces.device
    v, f = int(vertices.shape[0]), int(faces.shape[0])
    if v == 0 and f == 0:
        return empty_mesh_with_index(dev, return_index)
    ws, v2, f2, _ = _count(vertices, colors, faces, voxel, workspace)
    out_v = torch.empty((v2, 3), dtype=torch.float32, device=dev)
    out_c = torch.empty((v2, 3), dtype=torch.uint8, device=dev)
    out_f = torch.empty((f2, 3), dtype=torch.int32, device=dev)
    cluster_of = torch.empty((v,), dtype=torch.int64, device=dev) if return_index else None
    rows_f = torch.empty((f2,), dtype=torch.int64, device=dev) if return_index else None
    _ffi.call("m3_mesh_simplify_scatter", _ffi.ptr(vertices) if v else None, _ffi.ptr(colors) if v else None,
              _ffi.ptr(faces) if f else None, v, f, _ffi.ptr(ws), ws.numel(), v2, f2, _ffi.ptr(out_v) if v2 else None,
              _ffi.ptr(out_c) if v2 else None, _ffi.ptr(out_f) if f2 else None, _ffi.ptr(cluster_of) if v else None,
              _ffi.ptr(rows_f) if f2 else None, _ffi.stream_ptr())
    return (out_v, out_c, out_f, cluster_of, rows_f) if return_index else (out_v, out_c, out_f)
