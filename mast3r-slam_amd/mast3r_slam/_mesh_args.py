"""Argument handling shared by the mesh passes (components, simplify, smooth, normals) and, for the workspace, the cloud
passes: a mesh passed whole or unpacked, the dtype, shape and device checks, the workspace, the invalid-face error and
the empty result.  Shapes and dtypes raise ValueError before the first device check; a CPU tensor raises RuntimeError."""
from __future__ import annotations

from typing import Optional

import torch

from . import _ffi
from .export import _check_workspace, _empty_mesh

_WHOLE = "a mesh is (vertices, colors, faces[, index]), passed whole or unpacked"


def whole_or_unpacked_error() -> ValueError:
    return ValueError(_WHOLE)


def unpack_mesh(vertices, colors=None, faces=None):
    """(vertices, colors, faces) of a mesh passed unpacked, or whole as the tuple the producers return."""
    if isinstance(vertices, (tuple, list)):
        if len(vertices) < 3 or colors is not None or faces is not None:
            raise whole_or_unpacked_error()
        vertices, colors, faces = vertices[:3]
    return vertices, colors, faces


def _shape3(t, dtype, name: str) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != 2 or t.shape[1] != 3:
        got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{name} must be a {dtype} [n,3] tensor, got {got}")


def check_shape3(t, dtype, name: str) -> None:
    """ValueError unless t is a dtype [n,3] tensor; no device check."""
    _shape3(t, dtype, name)


def check_rows3(*named):
    """The (tensor, dtype, name) triples as contiguous device tensors: ValueError unless each is a dtype [n,3] tensor (all
    of them are looked at before the first device check), RuntimeError for a CPU tensor."""
    for t, dtype, name in named:
        _shape3(t, dtype, name)
    return [_ffi.check(t, dtype, name) for t, dtype, name in named]


def check_faces(faces, shape_checked: bool = False) -> torch.Tensor:
    """faces as a contiguous device tensor.  shape_checked: the caller has called check_shape3 on it already."""
    if not shape_checked:
        _shape3(faces, torch.int32, "faces")
    return _ffi.check(faces, torch.int32, "faces")


def check_mesh(vertices, colors, faces, rows_first: bool = False):
    """The three arrays of a mesh, checked: device tensors of the right dtype and shape, as many colours as vertices, on
    one device.  rows_first: the row counts of vertices and colours are compared before the faces are looked at (the
    order filter_components has always reported in)."""
    for t, dtype, name in ((vertices, torch.float32, "vertices"), (colors, torch.uint8, "colors")):
        _shape3(t, dtype, name)
    if not rows_first:
        _shape3(faces, torch.int32, "faces")
    if colors.shape[0] != vertices.shape[0]:
        raise ValueError(f"vertices has {vertices.shape[0]} rows, colors {colors.shape[0]}")
    _shape3(faces, torch.int32, "faces")
    faces = _ffi.check(faces, torch.int32, "faces")
    vertices, colors = _ffi.check(vertices, torch.float32, "vertices"), _ffi.check(colors, torch.uint8, "colors")
    dev = faces.device
    if vertices.device != dev or colors.device != dev:
        raise ValueError(f"faces live on {dev}, vertices on {vertices.device}, colors on {colors.device}")
    return vertices, colors, faces


def take_workspace(workspace: Optional[torch.Tensor], ws_bytes: int, device,
                   owner: Optional[str] = "the mesh lives") -> torch.Tensor:
    """The caller's workspace, checked - a contiguous, 16-byte aligned uint8 tensor of at least ws_bytes on `device` - or
    a new one.  owner None: the device is not compared (the view passes and the focal estimate never did)."""
    if workspace is None:
        workspace = torch.empty((ws_bytes,), dtype=torch.uint8, device=device)
    _check_workspace(workspace, ws_bytes)
    if owner is not None and workspace.device != device:
        raise ValueError(f"{owner} on {device}, the workspace on {workspace.device}")
    return workspace


def raise_invalid_faces(n: int, v: int) -> None:
    """ValueError when the header of a pass counted n > 0 faces with a row outside [0, v)."""
    if n:
        raise ValueError(f"{n} faces name a vertex row outside [0, {v})")


def empty_mesh_with_index(device, return_index: bool):
    """The empty mesh, and with return_index two empty int64 index tensors behind it."""
    mesh = _empty_mesh(device, False)
    if not return_index:
        return mesh
    return mesh + (torch.empty((0,), dtype=torch.int64, device=device), torch.empty((0,), dtype=torch.int64, device=device))
