"""Camera calibration: lens models, the undistortion table and the remap on the device in front of
preprocess.resize_img_device.

The calibrated operators (k_track_accum<Calib>, m3_constrain_points_to_ray, solve_GN_calib, render_map) assume an ideal
pinhole K; a real lens does not obey one.  The split is the one of preprocess.py: the host derives, in float64 and from
the calibration alone, a table of source coordinates in 1/256 pixel (`CameraModel.undistort_table`, cached), and
m3_remap_bilinear_u8 (csrc/undistort.hip) applies it with integer arithmetic: identical bytes every time.  The reference
has no undistortion (its use_calib takes a K from nowhere), so the rule is this project's own; tests/undistort_twin.py
restates it.  Integer pixel coordinates are pixel centres, as in render.hip and k_constrain_to_ray.

Everything above `undistort_device` is numpy on the host and needs no torch.  There is no host remap: a CPU tensor
raises like every other operator here.
"""
from __future__ import annotations

import functools
import json
import os
from typing import Mapping, Optional, Sequence

import numpy as np

PINHOLE, RADTAN, EQUIDISTANT = "pinhole", "radtan", "equidistant"
_COEFFS = {PINHOLE: (0,), RADTAN: (4, 5), EQUIDISTANT: (4,)}
FRAC_BITS = 8                                  # table entries are source coordinates times 2^8
COORD_LIMIT = float(1 << 20)                   # |source coordinate| at or past this becomes the sentinel
SENTINEL = np.iinfo(np.int32).min
INVERSE_TOL = 1e-10                            # |distort(undistort(p)) - p|, normalised coordinates
_MAX_NEWTON = 60
_POLISH_TOL = 1e-15                            # the Newton steps stop here, or where they stop helping


class CameraModel:
    """A camera of `width` x `height` pixels with pinhole K = [fx, fy, cx, cy] and a lens `model`:
    "radtan" (k1, k2, p1, p2[, k3]), "equidistant" (k1, k2, k3, k4) or "pinhole" (no coefficients).
    Immutable and hashable: tables are cached per camera."""

    def __init__(self, width: int, height: int, K: Sequence[float], distortion: Sequence[float] = (),
                 model: str = PINHOLE) -> None:
        if model not in _COEFFS:
            raise ValueError(f"unknown distortion model {model!r}: use one of {sorted(_COEFFS)}")
        K = tuple(float(v) for v in np.asarray(K, dtype=np.float64).reshape(-1))
        d = tuple(float(v) for v in np.asarray(distortion, dtype=np.float64).reshape(-1))
        if len(K) != 4:
            raise ValueError(f"K must be [fx, fy, cx, cy], got {len(K)} values")
        if len(d) not in _COEFFS[model]:
            raise ValueError(f"model {model!r} takes {' or '.join(map(str, _COEFFS[model]))} distortion coefficients, got {len(d)}")
        if int(width) < 1 or int(height) < 1 or not (K[0] > 0 and K[1] > 0) or not np.isfinite(K + d).all():
            raise ValueError(f"bad camera: size {width}x{height}, K {K}, distortion {d}")
        if model == RADTAN and len(d) == 4:
            d = d + (0.0,)
        self._key = (int(width), int(height), K, d, model)

    width = property(lambda self: self._key[0])
    height = property(lambda self: self._key[1])
    K = property(lambda self: self._key[2])
    distortion = property(lambda self: self._key[3])
    model = property(lambda self: self._key[4])

    def __hash__(self) -> int:
        return hash(self._key)

    def __eq__(self, other) -> bool:
        return isinstance(other, CameraModel) and self._key == other._key

    def __repr__(self) -> str:
        return f"CameraModel({self.width}, {self.height}, K={list(self.K)}, distortion={self.distortion}, model={self.model!r})"

    @property
    def has_distortion(self) -> bool:
        return self.model != PINHOLE and any(v != 0.0 for v in self.distortion)

    # ------------------------------------------------------------------ the lens, normalised coordinates
    def distort_points(self, xy) -> np.ndarray:
        """Ideal normalised coordinates [..., 2] -> distorted normalised coordinates, float64."""
        xy = np.asarray(xy, dtype=np.float64)
        if not self.has_distortion:
            return xy.copy()
        x, y = xy[..., 0], xy[..., 1]
        r2 = x * x + y * y
        if self.model == RADTAN:
            k1, k2, p1, p2, k3 = self.distortion
            rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
            xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        else:
            k1, k2, k3, k4 = self.distortion
            r = np.sqrt(r2)
            th = np.arctan(r)
            t2 = th * th
            thd = th * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
            with np.errstate(invalid="ignore", divide="ignore"):
                s = np.where(r > 0.0, thd / r, 1.0)
            xd, yd = x * s, y * s
        return np.stack([xd, yd], axis=-1)

    def undistort_points(self, xy, strict: bool = True) -> np.ndarray:
        """The inverse of distort_points by Newton iteration from the distorted point, until
        |distort(result) - xy| < 1e-10 in both coordinates.  A point that does not get there raises ValueError for the
        whole call, or comes back as NaN with strict=False; the iteration cap is never a silent stop."""
        target = np.asarray(xy, dtype=np.float64)
        if not self.has_distortion:
            return target.copy()
        shape = target.shape
        t = target.reshape(-1, 2)
        p = t.copy()
        h = 1e-6
        with np.errstate(all="ignore"):
            # the steps go on past the tolerance, to the floor of float64 (a step is kept where it lowers the residual),
            # so the answer does not sit just under 1e-10; the verdict below is against 1e-10 whatever ended the loop
            best = np.abs(self.distort_points(p) - t).max(axis=1)
            todo = ~(best < _POLISH_TOL) & np.isfinite(p).all(axis=1)
            for _ in range(_MAX_NEWTON):
                if not todo.any():
                    break
                q = p[todo]
                e = self.distort_points(q) - t[todo]
                jx = (self.distort_points(q + (h, 0.0)) - self.distort_points(q - (h, 0.0))) / (2.0 * h)
                jy = (self.distort_points(q + (0.0, h)) - self.distort_points(q - (0.0, h))) / (2.0 * h)
                det = jx[:, 0] * jy[:, 1] - jy[:, 0] * jx[:, 1]
                dx = (jy[:, 1] * e[:, 0] - jy[:, 0] * e[:, 1]) / det
                dy = (jx[:, 0] * e[:, 1] - jx[:, 1] * e[:, 0]) / det
                q = q - np.stack([dx, dy], axis=1)
                r = np.abs(self.distort_points(q) - t[todo]).max(axis=1)
                better = r < best[todo]
                idx = np.flatnonzero(todo)
                p[idx[better]], best[idx[better]] = q[better], r[better]
                # a point below the tolerance that stopped improving is done; one above it keeps stepping from the new place
                stuck = ~better & (best[idx] < INVERSE_TOL)
                p[idx[~better & ~stuck]] = q[~better & ~stuck]
                todo[idx[stuck]] = False
                todo &= ~(best < _POLISH_TOL) & np.isfinite(p).all(axis=1)
            bad = ~(np.abs(self.distort_points(p) - t).max(axis=1) < INVERSE_TOL)
        if bad.any():
            if strict:
                i = int(np.flatnonzero(bad)[0])
                raise ValueError(f"undistort_points: {int(bad.sum())} of {len(t)} points have no inverse within "
                                 f"{INVERSE_TOL:g} after {_MAX_NEWTON} Newton steps (first: {tuple(t[i])}) for {self!r}")
            p[bad] = np.nan
        return p.reshape(shape)

    # ------------------------------------------------------------------ the undistorted camera
    def new_camera_matrix(self, mode="inner", out_size=None):
        """[fx, fy, cx, cy] of the undistorted image of out_size = (W, H) (default: the source size).  "same": K.
        "inner": the largest axis-aligned rectangle of ideal coordinates inside the undistorted source border, i.e.
        every output pixel sees the source: x_l = max of the undistorted x over the pixel centres of the left border
        column, x_r = min over the right one, y_t / y_b likewise over the top and bottom rows; fx' = (W-1) / (x_r - x_l),
        cx' = -x_l fx', the same in y.  A border pixel without an inverse raises.  A 4-sequence is returned as given."""
        if not isinstance(mode, str):
            K_new = tuple(float(v) for v in np.asarray(mode, dtype=np.float64).reshape(-1))
            if len(K_new) != 4 or not (K_new[0] > 0 and K_new[1] > 0) or not np.isfinite(K_new).all():
                raise ValueError(f"K_new must be 'same', 'inner' or [fx, fy, cx, cy], got {mode!r}")
            return K_new
        wo, ho = (self.width, self.height) if out_size is None else (int(out_size[0]), int(out_size[1]))
        return _new_camera_matrix(self, mode, wo, ho)

    def undistort_table(self, K_new=None, out_size=None) -> np.ndarray:
        """int32 [Ho, Wo, 2], read-only, cached: entry (v, u) = (floor(sx 256 + 0.5), floor(sy 256 + 0.5)) with
        x = (u - cx') / fx', y = (v - cy') / fy', (xd, yd) = distort(x, y), sx = fx xd + cx, sy = fy yd + cy in float64;
        a non-finite coordinate or one with |s| >= 2^20 gives the sentinel (INT32_MIN, INT32_MIN).
        K_new: None = "inner", "same", "inner" or [fx, fy, cx, cy]; out_size = (W, H), default the source size."""
        wo, ho = (self.width, self.height) if out_size is None else (int(out_size[0]), int(out_size[1]))
        if wo < 1 or ho < 1:
            raise ValueError(f"out_size must be positive, got {(wo, ho)}")
        return _table(self, self.new_camera_matrix("inner" if K_new is None else K_new, (wo, ho)), wo, ho)


@functools.lru_cache(maxsize=64)
def _new_camera_matrix(cam: CameraModel, mode: str, wo: int, ho: int):
    if mode == "same" or (mode == "inner" and not cam.has_distortion):
        return cam.K
    if mode != "inner":
        raise ValueError(f"unknown new camera matrix {mode!r}: use 'same', 'inner' or [fx, fy, cx, cy]")
    fx, fy, cx, cy = cam.K
    us, vs = np.arange(cam.width, dtype=np.float64), np.arange(cam.height, dtype=np.float64)

    def column(u):
        return cam.undistort_points(np.stack([np.full_like(vs, (u - cx) / fx), (vs - cy) / fy], -1))[:, 0]

    def row(v):
        return cam.undistort_points(np.stack([(us - cx) / fx, np.full_like(us, (v - cy) / fy)], -1))[:, 1]

    x_l, x_r = column(0.0).max(), column(cam.width - 1.0).min()
    y_t, y_b = row(0.0).max(), row(cam.height - 1.0).min()
    if not (x_r > x_l and y_b > y_t):
        raise ValueError(f"no inner rectangle: x in [{x_l}, {x_r}], y in [{y_t}, {y_b}] for {cam!r}")
    fxn, fyn = max(wo - 1, 1) / (x_r - x_l), max(ho - 1, 1) / (y_b - y_t)
    return (float(fxn), float(fyn), float(-x_l * fxn), float(-y_t * fyn))


@functools.lru_cache(maxsize=8)
def _table(cam: CameraModel, K_new, wo: int, ho: int) -> np.ndarray:
    fx, fy, cx, cy = cam.K
    fxn, fyn, cxn, cyn = K_new
    u, v = np.meshgrid(np.arange(wo, dtype=np.float64), np.arange(ho, dtype=np.float64))
    with np.errstate(all="ignore"):
        d = cam.distort_points(np.stack([(u - cxn) / fxn, (v - cyn) / fyn], -1))
        s = np.stack([fx * d[..., 0] + cx, fy * d[..., 1] + cy], -1)
        ok = (np.isfinite(s) & (np.abs(s) < COORD_LIMIT)).all(axis=-1)
        q = np.floor(np.where(ok[..., None], s, 0.0) * float(1 << FRAC_BITS) + 0.5).astype(np.int64)
    q[~ok] = SENTINEL
    out = q.astype(np.int32)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------- calibration files
_EUROC_MODELS = {"radial-tangential": RADTAN, "radtan": RADTAN, "equidistant": EQUIDISTANT}


def _floats(v, what: str, source: str):
    try:
        return [float(x) for x in v]
    except (TypeError, ValueError):
        raise ValueError(f"{source}: `{what}` must be a list of numbers, got {v!r}") from None


def _from_mapping(m: Mapping, source: str) -> CameraModel:
    if not isinstance(m, Mapping):
        raise ValueError(f"{source}: expected a mapping of calibration keys, got {type(m).__name__}")
    try:
        if "distortion_model" in m or "resolution" in m:                     # EuRoC sensor.yaml
            for k in ("resolution", "intrinsics", "distortion_model", "distortion_coefficients"):
                if k not in m:
                    raise ValueError(f"{source}: EuRoC calibration lacks `{k}`")
            name = str(m["distortion_model"]).strip().lower()
            if name not in _EUROC_MODELS:
                raise ValueError(f"{source}: unknown distortion_model {m['distortion_model']!r}: "
                                 f"use one of {sorted(_EUROC_MODELS)}")
            w, h = (int(v) for v in m["resolution"])
            return CameraModel(w, h, _floats(m["intrinsics"], "intrinsics", source),
                               _floats(m["distortion_coefficients"], "distortion_coefficients", source), _EUROC_MODELS[name])
        for k in ("width", "height"):
            if k not in m:
                raise ValueError(f"{source}: calibration lacks `{k}`")
        w, h = int(m["width"]), int(m["height"])
        if "calibration" in m:                                               # the flat form: K then radtan coefficients
            c = _floats(m["calibration"], "calibration", source)
            if len(c) not in (4, 8, 9):
                raise ValueError(f"{source}: `calibration` holds 4 (pinhole), 8 or 9 (radtan) values, got {len(c)}")
            return CameraModel(w, h, c[:4], c[4:], RADTAN if len(c) > 4 else PINHOLE)
        if "intrinsics" not in m:
            raise ValueError(f"{source}: calibration lacks `intrinsics` (or the flat `calibration` list)")
        dist = _floats(m.get("distortion") or (), "distortion", source)
        model = str(m.get("model", RADTAN if dist else PINHOLE)).strip().lower()
        return CameraModel(w, h, _floats(m["intrinsics"], "intrinsics", source), dist, _EUROC_MODELS.get(model, model))
    except ValueError as e:
        if str(e).startswith(source):
            raise
        raise ValueError(f"{source}: {e}") from None


def load_calibration(src) -> CameraModel:
    """A CameraModel from a YAML / JSON file or a mapping, in one of three forms:
      this project's   width, height, model ("pinhole" | "radtan" | "equidistant"), intrinsics [fx, fy, cx, cy], distortion
      the flat form    width, height, calibration [fx, fy, cx, cy(, k1, k2, p1, p2(, k3))]
      EuRoC sensor.yaml  resolution [W, H], intrinsics, distortion_model (radial-tangential | equidistant),
                       distortion_coefficients
    Unknown models and wrong coefficient counts raise ValueError naming the file."""
    if isinstance(src, CameraModel):
        return src
    if isinstance(src, Mapping):
        return _from_mapping(src, "calibration mapping")
    path = os.fspath(src)
    with open(path) as f:
        text = f.read()
    try:
        if path.lower().endswith(".json"):
            data = json.loads(text)
        else:
            import yaml
            # OpenCV-style files open with a "%YAML:1.0" line that is no YAML directive
            data = yaml.safe_load("\n".join(l for l in text.splitlines() if not l.startswith("%YAML")))
    except Exception as e:
        raise ValueError(f"{path}: not a readable calibration file ({e})") from None
    return _from_mapping(data, path)


CALIBRATION_FILES = ("calibration.yaml", "calibration.json")


def find_calibration(directory) -> Optional[CameraModel]:
    """The calibration.yaml / calibration.json of a dataset directory, or None."""
    for name in CALIBRATION_FILES:
        p = os.path.join(os.fspath(directory), name)
        if os.path.isfile(p):
            return load_calibration(p)
    return None


# ---------------------------------------------------------------------- the device
# The uploaded tables stay alive with the process: 8 bytes per output pixel each (16.6 MB at 1920x1080), the 8 most
# recently used (camera, K_new, size, device); _device_table.cache_clear() drops them.
@functools.lru_cache(maxsize=8)
def _device_table(cam: CameraModel, K_new, wo: int, ho: int, device_index: int):
    import torch
    return torch.from_numpy(_table(cam, K_new, wo, ho).copy()).to(torch.device("cuda", device_index))


def prepare_undistort(cam: CameraModel, device, K_new="inner", out_size=None) -> None:
    """Builds and uploads the table that undistort_device(img, cam, K_new, out_size) on `device` will read.  The upload is
    a copy from pageable host memory, which has no place in a stream capture: call this (or undistort_device once)
    before capturing a graph that holds the launch."""
    import torch
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"prepare_undistort: must target the ROCm device (got {device})")
    wo, ho = (cam.width, cam.height) if out_size is None else (int(out_size[0]), int(out_size[1]))
    K_new = cam.new_camera_matrix("inner" if K_new is None else K_new, (wo, ho))
    if cam.has_distortion or K_new != cam.K or (wo, ho) != (cam.width, cam.height):
        _device_table(cam, K_new, wo, ho, device.index if device.index is not None else torch.cuda.current_device())


def remap_bilinear(src, table, border: int = 0):
    """src uint8 [B,Hs,Ws,3] and table int32 [Ho,Wo,2] on the device -> uint8 [B,Ho,Wo,3] (m3_remap_bilinear_u8)."""
    import torch

    from . import _ffi
    src = _ffi.check(src, torch.uint8, "src", (None, None, None, 3))
    table = _ffi.check(table, torch.int32, "table", (None, None, 2))
    if src.data_ptr() % 16:                           # a view at an odd storage offset
        src = src.clone()
    if table.data_ptr() % 16:
        table = table.clone()
    if not 0 <= int(border) <= 255:
        raise ValueError(f"border must be in 0 ... 255, got {border}")
    b, hs, ws, _ = src.shape
    ho, wo, _ = table.shape
    dst = torch.empty((b, ho, wo, 3), dtype=torch.uint8, device=src.device)
    _ffi.call("m3_remap_bilinear_u8", _ffi.ptr(src), _ffi.ptr(table), _ffi.ptr(dst), b, hs, ws, ho, wo, int(border),
              _ffi.stream_ptr())
    return dst


def undistort_device(img_u8, cam: CameraModel, K_new="inner", out_size=None, border: int = 0):
    """uint8 [H,W,3] or [B,H,W,3] on the device, taken by `cam` -> the image an ideal pinhole camera K_new
    (cam.new_camera_matrix(K_new, out_size)) of out_size = (W, H) would have taken, uint8 on the same device; pixels that
    see nothing of the source are `border`.  One launch; the table is uploaded once per (camera, K_new, size, device), by
    the first call, which therefore has to come before a stream capture (prepare_undistort does only that).
    A camera without distortion and K_new equal to its K returns the input without a launch."""
    import torch
    if not isinstance(img_u8, torch.Tensor):
        raise TypeError(f"img: expected a torch.Tensor, got {type(img_u8).__name__}")
    if img_u8.dim() not in (3, 4) or img_u8.shape[-1] != 3:
        raise ValueError(f"img: expected [H,W,3] or [B,H,W,3], got {tuple(img_u8.shape)}")
    if not img_u8.is_cuda:
        raise RuntimeError(f"img: must live on the ROCm device (got {img_u8.device}); no CPU path exists")
    if img_u8.dtype != torch.uint8:
        raise TypeError(f"img: expected torch.uint8, got {img_u8.dtype}")
    h, w = img_u8.shape[-3], img_u8.shape[-2]
    if (w, h) != (cam.width, cam.height):
        raise ValueError(f"the calibration is for {cam.width}x{cam.height} frames, this one is {w}x{h}")
    wo, ho = (w, h) if out_size is None else (int(out_size[0]), int(out_size[1]))
    K_new = cam.new_camera_matrix("inner" if K_new is None else K_new, (wo, ho))
    if not cam.has_distortion and K_new == cam.K and (wo, ho) == (w, h):
        return img_u8
    batched = img_u8.dim() == 4
    di = img_u8.device.index if img_u8.device.index is not None else torch.cuda.current_device()
    dst = remap_bilinear(img_u8 if batched else img_u8[None], _device_table(cam, K_new, wo, ho, di), border)
    return dst if batched else dst[0]
