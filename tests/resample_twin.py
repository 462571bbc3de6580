"""numpy statement of Pillow's 8-bit Image.resize (LANCZOS / BICUBIC) and of mast3r_utils.resize_img on top of it: the
yardstick of the device preprocessing tests.  It shares no code with mast3r_slam/preprocess.py;
tests/test_preprocess_host.py pins it to PIL byte for byte, so the GPU tests need not rely on PIL.

Rule, per axis, S = 3 (lanczos) or 2 (bicubic):
  scale = in / out, fs = max(scale, 1), support = S * fs, ksize = ceil(support) * 2 + 1
  center = (xx + 0.5) * scale, xmin = max(trunc(center - support + 0.5), 0), xmax = min(trunc(center + support + 0.5), in)
  w[x] = filter((x + xmin - center + 0.5) * (1 / fs)), x < xmax - xmin, divided by their sum (added in index order;
         the reciprocal is rounded first, as in Pillow - dividing by fs moves some arguments by one unit in the last place)
  k = trunc(w * 2^22 +- 0.5) (away from zero), out = clamp((2^21 + sum src * k) >> 22, 0, 255) in int32
Horizontal pass first (result rounded to uint8), then vertical; an axis whose size does not change has no pass.
"""
import math

import numpy as np

BITS = 22


def _filter(kind):
    def sinc(x):
        if x == 0.0:
            return 1.0
        x = x * math.pi
        return math.sin(x) / x

    def lanczos(x):
        return sinc(x) * sinc(x / 3) if -3.0 <= x < 3.0 else 0.0

    def bicubic(x, a=-0.5):
        x = abs(x)
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0

    return {"lanczos": (lanczos, 3.0), "bicubic": (bicubic, 2.0)}[kind]


def coeffs(in_size, out_size, kind):
    """-> (bounds int32 [out,2] = (xmin, n), k int32 [out,ksize])."""
    f, s = _filter(kind)
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = s * fs
    ksize = int(math.ceil(support)) * 2 + 1
    inv = 1.0 / fs                                     # Pillow multiplies by the reciprocal
    bounds = np.zeros((out_size, 2), np.int32)
    k = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        w = [f((x + xmin - center + 0.5) * inv) for x in range(xmax - xmin)]
        tot = 0.0
        for v in w:
            tot += v
        if tot != 0.0:
            w = [v / tot for v in w]
        bounds[xx] = (xmin, xmax - xmin)
        k[xx, :len(w)] = [int(v * (1 << BITS) + (0.5 if v >= 0 else -0.5)) for v in w]
    return bounds, k


def _pass(a, bounds, k):
    """Resample axis 0 of uint8 a [n, ...] -> [out, ...]."""
    out = np.empty((bounds.shape[0],) + a.shape[1:], np.uint8)
    for o, (xmin, n) in enumerate(bounds):
        acc = np.tensordot(k[o, :n].astype(np.int64), a[xmin:xmin + n].astype(np.int64), axes=(0, 0)) + (1 << (BITS - 1))
        assert np.abs(acc).max() < 1 << 31
        out[o] = np.clip(acc >> BITS, 0, 255).astype(np.uint8)
    return out


def resize(a, size_wh, kind):
    """uint8 [H,W,3] -> [size_wh[1], size_wh[0], 3], as PIL.Image.resize(size_wh, LANCZOS | BICUBIC)."""
    a = np.ascontiguousarray(a)
    w, h = size_wh
    if w != a.shape[1]:
        a = _pass(a.transpose(1, 0, 2), *coeffs(a.shape[1], w, kind)).transpose(1, 0, 2)
    if h != a.shape[0]:
        a = _pass(a, *coeffs(a.shape[0], h, kind))
    return np.ascontiguousarray(a)


def geometry(h1, w1, size, square_ok=False):
    """Resized (W, H), filter kind and crop box of resize_img for an [h1, w1] source."""
    long_edge = round(size * max(w1 / h1, h1 / w1)) if size == 224 else size
    s = max(w1, h1)
    kind = "lanczos" if s > long_edge else "bicubic"
    w, h = int(round(w1 * long_edge / s)), int(round(h1 * long_edge / s))
    cx, cy = w // 2, h // 2
    if size == 224:
        half = min(cx, cy)
        return (w, h), kind, (cx - half, cy - half, cx + half, cy + half)
    halfw, halfh = ((2 * cx) // 16) * 8, ((2 * cy) // 16) * 8
    if not square_ok and w == h:
        halfh = int(3 * halfw / 4)
    return (w, h), kind, (cx - halfw, cy - halfh, cx + halfw, cy + halfh)


def resize_img(a, size, square_ok=False):
    """uint8 [H,W,3] -> (unnormalized_img uint8 [H',W',3], img float32 [1,H',W',3]) of mast3r_utils.resize_img."""
    wh, kind, (x0, y0, x1, y1) = geometry(a.shape[0], a.shape[1], size, square_ok)
    raw = np.ascontiguousarray(resize(a, wh, kind)[y0:y1, x0:x1])
    return raw, ((raw.astype(np.float32) / 255.0 - 0.5) / 0.5)[None]


def make_content(kind, h, w, seed=0):
    """Test images uint8 [h,w,3]: "noise", "smooth" ramps, or "extreme" (0 / 255 only: clamps and negative lobes)."""
    y, x = np.mgrid[0:h, 0:w]
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "smooth":
        return np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) % 256], -1).astype(np.uint8)
    return (np.stack([(x // 3 + y // 2) % 2, (x + y) % 2, (x // 7) % 2], -1) * 255).astype(np.uint8)   # 0 / 255 only
