"""Frame preprocessing on the device: the resize + centre crop of mast3r_utils.resize_img (mast3r_utils.py:132-207 of
the reference) as one HIP launch in front of patchify16, bit for bit what Pillow computes on the host.

Pillow's 8-bit resampling is integer arithmetic on fixed-point coefficients that the host derives in float64 from the
two sizes alone, so the split is: `resize_geometry` (the integer logic of resize_img), `resample_tables` (the
coefficients, cached per (in, out, kind)) and m3_resize_crop_u8 (csrc/preprocess.hip: the two passes and the crop).
There is no host fallback: a CPU tensor raises like every other operator here.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from . import _ffi

LANCZOS, BICUBIC = "lanczos", "bicubic"
_SUPPORT = {LANCZOS: 3.0, BICUBIC: 2.0}
PRECISION_BITS = 22                      # 32 - 8 - 2: an 8-bit sample times a coefficient, summed, stays inside int32


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x: float) -> float:
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_FILTER = {LANCZOS: _lanczos, BICUBIC: _bicubic}


def check_tables(k: np.ndarray) -> None:
    """int32 accumulation of a pass is safe when 255 * sum|k| + 2^21 < 2^31 for every output index; the kernel forms
    the products with the 24-bit multiplier, which is exact for |k| < 2^23."""
    worst = int(np.abs(k.astype(np.int64)).sum(axis=1).max()) if k.size else 0
    if k.size and int(np.abs(k.astype(np.int64)).max()) >= 1 << 23:
        raise ValueError("resample coefficients overflow the 24-bit multiplier: |k| >= 2^23")
    if 255 * worst + (1 << (PRECISION_BITS - 1)) >= 1 << 31:
        raise ValueError(f"resample coefficients overflow int32 accumulation: 255 * {worst} + 2^21 >= 2^31")


@functools.lru_cache(maxsize=64)
def _tables(in_size: int, out_size: int, kind: str):
    if kind not in _FILTER:
        raise ValueError(f"unknown filter {kind!r}: use {LANCZOS!r} or {BICUBIC!r}")
    if in_size < 1 or out_size < 1:
        raise ValueError(f"sizes must be positive, got {in_size} -> {out_size}")
    filt = _FILTER[kind]
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support = _SUPPORT[kind] * fscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fscale
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    k = np.zeros((out_size, ksize), dtype=np.int32)
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w = [filt((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:                                   # summed in index order
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, n)
        for x, v in enumerate(w):
            k[xx, x] = int(v * one - 0.5) if v < 0 else int(v * one + 0.5)
    check_tables(k)
    bounds.setflags(write=False)
    k.setflags(write=False)
    return bounds, k


def resample_tables(in_size: int, out_size: int, kind: str):
    """-> (bounds int32 [out, 2] = (first source index, tap count), k int32 [out, ksize] fixed-point coefficients in
    units of 2^-22, zero past the tap count).  float64 throughout with math.sin - the libm Pillow itself calls; a
    vectorised sine may differ in the last bit and move a coefficient by one unit.  Cached; the arrays are read-only."""
    return _tables(int(in_size), int(out_size), kind)


def resize_geometry(h1: int, w1: int, size: int, square_ok: bool = False):
    """The integer logic of resize_img as a pure function of the source shape:
    -> ((W, H) of the resized image, filter kind, crop box (left, top, right, bottom) inside it,
        transformation (scale_w, scale_h, half_crop_w, half_crop_h))."""
    h1, w1 = int(h1), int(w1)
    if h1 < 1 or w1 < 1:
        raise ValueError(f"bad source shape {(h1, w1)}")
    long_edge = round(size * max(w1 / h1, h1 / w1)) if size == 224 else size
    s = max(w1, h1)
    kind = LANCZOS if s > long_edge else BICUBIC
    w, h = (int(round(x * long_edge / s)) for x in (w1, h1))
    if w < 1 or h < 1:
        raise ValueError(f"source shape {(h1, w1)} resizes to an empty image")
    cx, cy = w // 2, h // 2
    if size == 224:
        half = min(cx, cy)
        box = (cx - half, cy - half, cx + half, cy + half)
    else:
        halfw, halfh = ((2 * cx) // 16) * 8, ((2 * cy) // 16) * 8
        if not square_ok and w == h:
            halfh = int(3 * halfw / 4)
        box = (cx - halfw, cy - halfh, cx + halfw, cy + halfh)
    wc, hc = box[2] - box[0], box[3] - box[1]
    if wc < 1 or hc < 1:
        raise ValueError(f"source shape {(h1, w1)} leaves an empty crop at size {size}")
    return (w, h), kind, box, (w1 / w, h1 / h, (w - wc) / 2, (h - hc) / 2)


@functools.lru_cache(maxsize=32)
def _device_tables(in_size: int, out_size: int, kind: str, tap_major: bool, device_index: int):
    """The tables of one axis on the device, uploaded once per source shape (None when the axis is not resampled)."""
    if in_size == out_size:
        return None, None, 1
    bounds, k = resample_tables(in_size, out_size, kind)
    dev = torch.device("cuda", device_index)
    kk = np.ascontiguousarray(k.T) if tap_major else k
    return torch.from_numpy(bounds.copy()).to(dev), torch.from_numpy(kk.copy()).to(dev), k.shape[1]


@functools.lru_cache(maxsize=32)
def _true_shape(h: int, w: int, device_index: int) -> torch.Tensor:
    return torch.tensor([[h, w]], dtype=torch.int32, device=torch.device("cuda", device_index))


def resize_crop(src: torch.Tensor, out_wh, kind: str, box, want_float: bool = True):
    """src uint8 [B,Hs,Ws,3] on the device -> (uint8 [B,Hc,Wc,3], float32 [B,Hc,Wc,3] or None): src resampled to
    out_wh = (W, H) with Pillow's 8-bit arithmetic, then cropped to box = (left, top, right, bottom)."""
    src = _ffi.check(src, torch.uint8, "src", (None, None, None, 3))
    if src.data_ptr() % 16:                           # a view at an odd storage offset: the kernel stages 16-byte pieces
        src = src.clone()
    b, hs, ws, _ = src.shape
    wr, hr = int(out_wh[0]), int(out_wh[1])
    x0, y0, x1, y1 = (int(v) for v in box)
    di = src.device.index if src.device.index is not None else torch.cuda.current_device()
    bh, kh, ksh = _device_tables(ws, wr, kind, True, di)
    bv, kv, ksv = _device_tables(hs, hr, kind, False, di)
    dst = torch.empty((b, y1 - y0, x1 - x0, 3), dtype=torch.uint8, device=src.device)
    img = torch.empty(dst.shape, dtype=torch.float32, device=src.device) if want_float else None
    _ffi.call("m3_resize_crop_u8", _ffi.ptr(src), _ffi.ptr(bh), _ffi.ptr(kh), ksh, _ffi.ptr(bv), _ffi.ptr(kv), ksv,
              _ffi.ptr(dst), _ffi.ptr(img), b, hs, ws, hr, wr, x0, y0, y1 - y0, x1 - x0, _ffi.stream_ptr())
    return dst, img


def resize_img_device(img_u8: torch.Tensor, size: int = 512, square_ok: bool = False,
                      return_transformation: bool = False):
    """resize_img on the device: uint8 [H,W,3] or [B,H,W,3] -> dict(img float32 [B,H',W',3] in [-1,1], true_shape int32
    [[H',W']], unnormalized_img uint8 [H',W',3] / [B,H',W',3]) with device tensors, every byte and float bit equal to
    resize_img on the same frame.  Float sources are not taken (convert first: the host rule tests max() <= 1)."""
    if not isinstance(img_u8, torch.Tensor):
        raise TypeError(f"img: expected a torch.Tensor, got {type(img_u8).__name__}")
    if img_u8.dim() not in (3, 4) or img_u8.shape[-1] != 3:
        raise ValueError(f"img: expected [H,W,3] or [B,H,W,3], got {tuple(img_u8.shape)}")
    batched = img_u8.dim() == 4
    src = img_u8 if batched else img_u8[None]
    out_wh, kind, box, tf = resize_geometry(src.shape[1], src.shape[2], size, square_ok)
    dst, img = resize_crop(src, out_wh, kind, box)
    res = {"img": img,
           # a device copy of a cached tensor: no host-to-device transfer per call (one could not be graph-captured)
           "true_shape": _true_shape(dst.shape[1], dst.shape[2], dst.device.index).clone(),
           "unnormalized_img": dst if batched else dst[0]}
    if return_transformation:
        return res, tf
    return res


def adjust_intrinsics(K, transformation):
    """Intrinsics of the resized and cropped image: fx' = fx / scale_w, cx' = cx / scale_w - half_crop_w, same in y.
    K: [fx, fy, cx, cy] or a 3x3 matrix (tensor, array or sequence); the same form comes back."""
    sw, sh, cw, ch = (float(v) for v in transformation)
    is_t = isinstance(K, torch.Tensor)
    out = K.clone() if is_t else np.array(K, dtype=np.float64)
    if tuple(out.shape) == (4,):
        out[0], out[1] = out[0] / sw, out[1] / sh
        out[2], out[3] = out[2] / sw - cw, out[3] / sh - ch
    elif tuple(out.shape) == (3, 3):
        out[0, 0], out[1, 1] = out[0, 0] / sw, out[1, 1] / sh
        out[0, 2], out[1, 2] = out[0, 2] / sw - cw, out[1, 2] / sh - ch
        out[0, 1] = out[0, 1] / sw                    # skew scales with x
    else:
        raise ValueError(f"K must be [fx, fy, cx, cy] or 3x3, got shape {tuple(out.shape)}")
    return out
