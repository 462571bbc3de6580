"""Host side of the staged undistortion experiment (undistort_staged.hip, beside this file): the build recipe, the
per-tile source boxes and the call.  Not part of the package; tools/bench_undistort.py and
tests/test_gpu_undistort_staged.py use it.

    python tools/experiments/undistort_staged.py          # compile for gfx950 -> tools/experiments/_build/
"""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "undistort_staged.hip")
LIB = os.path.join(HERE, "_build", "libundistort_staged.so")
TILE_W, TILE_H = 64, 4
LDS_BYTES = 8192
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-shared"]


def build(force: bool = False, extra=()) -> str:
    """hipcc undistort_staged.hip -> _build/libundistort_staged.so (skipped when the object is newer than the source)."""
    if not force and os.path.exists(LIB) and os.path.getmtime(LIB) >= os.path.getmtime(SRC):
        return LIB
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    tmp = f"{LIB}.{os.getpid()}.tmp"
    r = subprocess.run([hipcc, *FLAGS, *extra, SRC, "-o", tmp], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {SRC}:\n{r.stderr}")
    os.replace(tmp, LIB)
    return LIB


def tile_boxes(table: np.ndarray, hs: int, ws: int) -> np.ndarray:
    """int32 [tiles_y * tiles_x, 4] = (x0, y0, w, h) in source pixels: the bounding box of the taps of each 64 x 4 tile of
    `table` (int32 [Ho, Wo, 2]).  A tile with a sentinel or with a tap outside the hs x ws source gets (0, 0, 0, 0), which
    the kernel does not stage."""
    q = np.asarray(table).astype(np.int64)
    ho, wo, _ = q.shape
    ty, tx = -(-ho // TILE_H), -(-wo // TILE_W)
    ix, iy = q[..., 0] >> 8, q[..., 1] >> 8
    pad = ((0, ty * TILE_H - ho), (0, tx * TILE_W - wo))
    tiles = lambda a: np.pad(a, pad, mode="edge").reshape(ty, TILE_H, tx, TILE_W)
    x0, x1 = tiles(ix).min(axis=(1, 3)), tiles(ix).max(axis=(1, 3)) + 1
    y0, y1 = tiles(iy).min(axis=(1, 3)), tiles(iy).max(axis=(1, 3)) + 1
    ok = (x0 >= 0) & (x1 < ws) & (y0 >= 0) & (y1 < hs)                 # a sentinel is far below zero
    box = np.stack([x0, y0, x1 - x0 + 1, y1 - y0 + 1], -1)
    box[~ok] = 0
    return np.ascontiguousarray(box.reshape(-1, 4).astype(np.int32))


def staged_share(boxes: np.ndarray) -> float:
    """The share of tiles the kernel stages: a box that is not empty and fits the LDS budget (the kernel's own test)."""
    w, h = boxes[:, 2].astype(np.int64), boxes[:, 3].astype(np.int64)
    pitch = ((w * 3 + 30) >> 4) << 4
    return float(((w >= 2) & (h >= 2) & (pitch * h <= LDS_BYTES)).mean())


_lib = None


def remap_staged(src, table, boxes, border: int = 0):
    """src uint8 [B,Hs,Ws,3], table int32 [Ho,Wo,2], boxes int32 [tiles,4] on the device -> uint8 [B,Ho,Wo,3]."""
    import torch
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
        _lib.exp_remap_staged_u8.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 6 + [ctypes.c_void_p]
        _lib.exp_remap_staged_u8.restype = ctypes.c_int
    assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous() and src.dim() == 4 and src.shape[-1] == 3
    assert table.is_cuda and table.dtype == torch.int32 and table.is_contiguous() and table.shape[-1] == 2
    assert boxes.is_cuda and boxes.dtype == torch.int32 and boxes.is_contiguous()
    b, hs, ws, _ = src.shape
    ho, wo, _ = table.shape
    if tuple(boxes.shape) != (-(-ho // TILE_H) * -(-wo // TILE_W), 4):
        raise ValueError(f"boxes {tuple(boxes.shape)} do not belong to a {wo}x{ho} table")
    if src.data_ptr() % 16:
        src = src.clone()
    dst = torch.empty((b, ho, wo, 3), dtype=torch.uint8, device=src.device)
    rc = _lib.exp_remap_staged_u8(src.data_ptr(), table.data_ptr(), boxes.data_ptr(), dst.data_ptr(), b, hs, ws, ho, wo,
                                  int(border), torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError(f"exp_remap_staged_u8 returned {rc}")
    return dst


if __name__ == "__main__":
    print(build(force=True))
