"""Edge topology of a triangle mesh and Laplacian / Taubin smoothing on the device (csrc/mesh_smooth.hip, DESIGN.md
section 7n).

A keyframe mesh carries the per-pixel noise of its pointmap and a surface-nets mesh the staircase of its voxel grid.
smooth_mesh is Open3D's filter_smooth_laplacian / filter_smooth_taubin (uniform weights) with the order of every sum
fixed, so that the mesh does not have to leave the device for it; mesh_topology answers what the smoothing needs
underneath - which vertices share an edge - and with it: is the mesh closed, how many boundary and non-manifold edges?

    edges              the undirected pairs of every face's rows; (a, a) is no edge; an edge is (lo, hi) by row; its
                       faces_of counts the face corners that contribute it (a repeated face counts every time); 1 is a
                       boundary edge, more than 2 a non-manifold one; a boundary vertex lies on a boundary edge
    adjacency          per vertex the other ends of its unique edges in ascending order: canonical, whatever the order
                       of the faces
    one pass, weight w a pinned vertex, one that is not finite and one without a finite neighbour keep their bits; any
                       other moves to p + w * (mean of its finite neighbours - p), summed in ascending row order in
                       float64, from the positions before the pass
    laplacian          `iterations` passes with lam;  taubin: `iterations` times a pass with lam, then one with mu

The exact rule is in include/m3slam.h.  Everything up to the adjacency is integer work whose result does not depend on
the execution order, and a pass adds in a fixed order: two calls give identical bytes, and so do two orders of the
face rows.  Cotangent and other geometric weights, smoothing of colours or normals (recompute normals with
vertex_normals), feature-preserving or bilateral filters, hole filling and a `smooth=` argument on the driver methods
are left out.  CPU tensors raise RuntimeError: there is no CPU path.
"""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from . import _ffi
from ._mesh_args import check_faces, check_mesh, check_shape3, raise_invalid_faces, take_workspace, unpack_mesh

__all__ = ["smooth_mesh", "mesh_topology", "MeshTopology", "workspace_bytes"]

MeshTopology = namedtuple("MeshTopology", ["edges", "boundary_edges", "nonmanifold_edges", "invalid_faces", "degree",
                                           "boundary", "edge_rows", "edge_faces"])
MeshTopology.__doc__ = ("edges, boundary_edges (one face), nonmanifold_edges (more than two faces), invalid_faces: counts; "
                        "degree int32 [V]: the unique neighbours of every vertex; boundary bool [V]: on a boundary edge; "
                        "edge_rows int32 [E,2] in (lo, hi) order and edge_faces int32 [E] with return_edges, else None.")

METHODS = {"laplacian": 0, "taubin": 1}
MAX_VERTICES = 2 ** 31 - 1                                              # include/m3slam.h
MAX_FACES = (2 ** 31 - 1) // 6
_HDR_WORDS = 4                                                          # 2 E, boundary edges, non-manifold edges, invalid faces


def workspace_bytes(n_vertices: int, n_faces: int) -> int:
    """Bytes of the workspace mesh_topology and smooth_mesh need for a mesh of n_vertices and n_faces."""
    b = int(_ffi.lib().m3_mesh_smooth_ws_bytes(int(n_vertices), int(n_faces)))
    if b <= 0:
        raise ValueError(f"unsupported mesh of {n_vertices} vertices (0 ... 2^31 - 1) and {n_faces} faces (0 ... (2^31 - 1) / 6)")
    return b


def _build(faces: torch.Tensor, v: int, ws: torch.Tensor) -> None:
    f = int(faces.shape[0])
    _ffi.call("m3_mesh_topology_build", _ffi.ptr(faces) if f else None, v, f, _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr())


def mesh_topology(faces, n_vertices: int, return_edges: bool = False, workspace: Optional[torch.Tensor] = None) -> MeshTopology:
    """MeshTopology(edges, boundary_edges, nonmanifold_edges, invalid_faces, degree, boundary, edge_rows, edge_faces) of
    the faces int32 [F,3] (a device tensor) over n_vertices vertices.

    A mesh is closed when boundary_edges == 0 and a manifold when also nonmanifold_edges == 0; `boundary` marks the rim
    of its holes.  return_edges adds the edges as int32 [E,2] rows (lo, hi) in lexicographic order and, per edge, the
    number of face corners on it.  The call queues 8 launches (11 with return_edges) and reads one 16-byte header back
    in between: its only synchronisation.  workspace: a 16-byte aligned uint8 device tensor of
    workspace_bytes(n_vertices, F).  ValueError when a face names a row outside [0, n_vertices); RuntimeError for a
    CPU tensor."""
    check_shape3(faces, torch.int32, "faces")                            # reported before a bad n_vertices, the device after it
    v = int(n_vertices)
    if v < 0 or v > MAX_VERTICES:
        raise ValueError(f"n_vertices must lie in 0 ... 2^31 - 1, got {n_vertices}")
    faces = check_faces(faces, shape_checked=True)
    dev, f = faces.device, int(faces.shape[0])
    ws = take_workspace(workspace, workspace_bytes(v, f), dev)
    _build(faces, v, ws)
    two_e, n_boundary, n_nonmanifold, invalid = ws[:4 * _HDR_WORDS].view(torch.int32).tolist()     # the one synchronisation
    raise_invalid_faces(invalid, v)
    e = two_e // 2
    degree = torch.empty((v,), dtype=torch.int32, device=dev)
    boundary = torch.empty((v,), dtype=torch.bool, device=dev)
    _ffi.call("m3_mesh_topology_read", _ffi.ptr(ws), v, f, _ffi.ptr(degree) if v else None, _ffi.ptr(boundary) if v else None,
              _ffi.stream_ptr())
    rows = counts = None
    if return_edges:
        rows = torch.empty((e, 2), dtype=torch.int32, device=dev)
        counts = torch.empty((e,), dtype=torch.int32, device=dev)
        _ffi.call("m3_mesh_topology_edges", _ffi.ptr(ws), v, f, e, _ffi.ptr(rows) if e else None, _ffi.ptr(counts) if e else None,
                  _ffi.stream_ptr())
    return MeshTopology(e, n_boundary, n_nonmanifold, invalid, degree, boundary, rows, counts)


def _weights(iterations, method, lam, mu):
    """(iterations, method number, lam, mu) checked, lam and mu rounded to fp32: ValueError before any device call."""
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 0 or iterations >= 2 ** 30:
        raise ValueError(f"iterations must be an integer >= 0, got {iterations!r}")
    if method not in METHODS:
        raise ValueError(f"method must be one of {tuple(METHODS)}, got {method!r}")
    with np.errstate(over="ignore"):
        lam32, mu32 = float(np.float32(lam)), float(np.float32(mu))
    if not math.isfinite(lam32) or not 0.0 < lam32 <= 1.0:
        raise ValueError(f"lam must lie in (0, 1] (as fp32), got {lam}")
    if not math.isfinite(mu32):
        raise ValueError(f"mu must be finite (as fp32), got {mu}")
    return int(iterations), METHODS[method], lam32, mu32


def smooth_mesh(vertices, colors=None, faces=None, iterations: int = 10, method: str = "taubin", lam: float = 0.5,
                mu: float = -0.53, fix_boundary: bool = False, pinned: Optional[torch.Tensor] = None,
                workspace: Optional[torch.Tensor] = None):
    """(vertices' float32 [V,3], colors, faces) of the mesh smoothed on the device; vertices' is a new tensor, colors and
    faces are the input tensors.  The mesh is passed unpacked or as the tuple export.collect_mesh, SLAM.mesh,
    fusion.extract_surface, SLAM.fused_mesh, filter_components or simplify_mesh return: smooth_mesh(slam.fused_mesh()).
    The result drops into vertex_normals, render_mesh, save_ply_mesh, filter_components and simplify_mesh.

    method "taubin" (the default) runs `iterations` times a pass with lam and a pass with mu, which removes ripples
    without shrinking the surface; "laplacian" runs `iterations` passes with lam and shrinks.  lam = 0.5 and mu = -0.53
    are Open3D's defaults; iterations = 10 is this project's choice and has not been tuned on real data.  A pass moves
    every vertex towards the mean of its edge neighbours by the weight, from the positions before the pass; vertices
    that are not finite stay as they are and count as no one's neighbour.  fix_boundary pins the vertices on a boundary
    edge - the rim of a keyframe mesh and of every hole; pinned: a bool [V] device tensor of further vertices that stay.
    iterations = 0 returns a copy.

    Nothing is read back, so a face with a row outside [0, V) contributes no edge (as in vertex_normals) and is no
    error: mesh_topology raises for it.  With a caller's workspace - a 16-byte aligned uint8 device tensor of
    workspace_bytes(V, F) - the call can be captured into a graph.  It queues 7 launches for the topology and one per
    pass.  Identical bytes on every call and for any order of the face rows.  ValueError for iterations < 0, an unknown
    method, a lam or mu that is not finite as fp32, a lam outside (0, 1] and a mask of the wrong shape, dtype or
    device; RuntimeError for CPU tensors."""
    iterations, m, lam32, mu32 = _weights(iterations, method, lam, mu)
    if pinned is not None and (not isinstance(pinned, torch.Tensor) or pinned.dtype != torch.bool or pinned.dim() != 1):
        got = f"{pinned.dtype} {tuple(pinned.shape)}" if isinstance(pinned, torch.Tensor) else type(pinned).__name__
        raise ValueError(f"pinned must be a {torch.bool} [V] tensor, got {got}")
    whole = isinstance(vertices, (tuple, list)) and len(vertices) >= 3
    mesh_colors, mesh_faces = (vertices[1], vertices[2]) if whole else (colors, faces)      # handed back as they came
    vertices, _, faces_c = check_mesh(*unpack_mesh(vertices, colors, faces))
    dev = faces_c.device
    v, f = int(vertices.shape[0]), int(faces_c.shape[0])
    if pinned is not None:
        if pinned.shape[0] != v:
            raise ValueError(f"vertices has {v} rows, pinned {pinned.shape[0]}")
        if pinned.device != dev:
            raise ValueError(f"the mesh lives on {dev}, pinned on {pinned.device}")
        pinned = pinned.contiguous()
    out = torch.empty((v, 3), dtype=torch.float32, device=dev)
    if v == 0:
        return out, mesh_colors, mesh_faces
    ws = take_workspace(workspace, workspace_bytes(v, f), dev)
    _build(faces_c, v, ws)
    _ffi.call("m3_mesh_smooth_passes", _ffi.ptr(vertices), v, f, _ffi.ptr(ws), ws.numel(), _ffi.ptr(pinned), 1 if fix_boundary else 0,
              m, iterations, lam32, mu32, _ffi.ptr(out), _ffi.stream_ptr())
    return out, mesh_colors, mesh_faces
