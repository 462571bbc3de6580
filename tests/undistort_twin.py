"""numpy statement of the undistortion remap (m3_remap_bilinear_u8) and of the table it reads: the yardstick of the
device tests.  It shares no code with mast3r_slam/camera.py; tests/test_camera_host.py pins it to the meaning of the
camera model (a smooth image seen through the lens comes back at its ideal position).

Table, float64: for output pixel (u, v) of a pinhole camera (fx', fy', cx', cy'), integer coordinates = pixel centres,
  x = (u - cx') / fx', y = (v - cy') / fy', (xd, yd) = distort(x, y), sx = fx xd + cx, sy = fy yd + cy
  entry = (floor(sx 256 + 0.5), floor(sy 256 + 0.5)); non-finite or |s| >= 2^20 -> (INT32_MIN, INT32_MIN)
radtan (k1, k2, p1, p2, k3), r2 = x^2 + y^2, rad = 1 + r2 (k1 + r2 (k2 + r2 k3)):
  xd = x rad + 2 p1 x y + p2 (r2 + 2 x^2), yd = y rad + p1 (r2 + 2 y^2) + 2 p2 x y
equidistant (k1..k4), r = sqrt(r2), th = atan(r), thd = th (1 + k1 th^2 + k2 th^4 + k3 th^6 + k4 th^8):
  xd = x thd / r, yd = y thd / r (xd = x, yd = y at r = 0)
Remap, int64: ix = qx >> 8, iy = qy >> 8 (floor), a = qx & 255, b = qy & 255,
  out = (p00 (256-a)(256-b) + p01 a (256-b) + p10 (256-a) b + p11 a b + 2^15) >> 16 per channel,
  p00 = src[iy][ix], p01 at ix+1, p10 at iy+1, p11 at both; a tap outside the source reads `border`.
"""
import numpy as np

SENTINEL = -(1 << 31)


def distort(model, dist, x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if model == "pinhole" or not len(dist):
        return x, y
    r2 = x * x + y * y
    if model == "radtan":
        k1, k2, p1, p2 = dist[:4]
        k3 = dist[4] if len(dist) > 4 else 0.0
        rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
        return x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    assert model == "equidistant"
    k1, k2, k3, k4 = dist
    r = np.sqrt(r2)
    th = np.arctan(r)
    thd = th * (1 + k1 * th ** 2 + k2 * th ** 4 + k3 * th ** 6 + k4 * th ** 8)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(r > 0, thd / r, 1.0)
    return x * s, y * s


def source_coords(model, K, dist, K_new, out_wh):
    """float64 (sx, sy), each [Ho, Wo]: where output pixel (u, v) of camera K_new looks in the source image."""
    fx, fy, cx, cy = K
    fxn, fyn, cxn, cyn = K_new
    u, v = np.meshgrid(np.arange(out_wh[0], dtype=np.float64), np.arange(out_wh[1], dtype=np.float64))
    xd, yd = distort(model, dist, (u - cxn) / fxn, (v - cyn) / fyn)
    return fx * xd + cx, fy * yd + cy


def table(model, K, dist, K_new, out_wh):
    sx, sy = source_coords(model, K, dist, K_new, out_wh)
    ok = np.isfinite(sx) & np.isfinite(sy) & (np.abs(sx) < 2.0 ** 20) & (np.abs(sy) < 2.0 ** 20)
    q = np.full(sx.shape + (2,), SENTINEL, np.int64)
    q[..., 0][ok] = np.floor(sx[ok] * 256 + 0.5)
    q[..., 1][ok] = np.floor(sy[ok] * 256 + 0.5)
    q[~ok] = SENTINEL
    return q.astype(np.int32)


def taps_inside(tab, hs, ws):
    """bool [Ho, Wo]: the four taps of the entry are all inside the source."""
    ix, iy = tab[..., 0].astype(np.int64) >> 8, tab[..., 1].astype(np.int64) >> 8
    return (ix >= 0) & (ix + 1 < ws) & (iy >= 0) & (iy + 1 < hs)


def remap(src, tab, border=0):
    """src uint8 [Hs,Ws,3] or [B,Hs,Ws,3], tab int32 [Ho,Wo,2] -> uint8 [Ho,Wo,3] / [B,Ho,Wo,3]."""
    src = np.asarray(src)
    if src.ndim == 4:
        return np.stack([remap(s, tab, border) for s in src])
    hs, ws, _ = src.shape
    q = np.asarray(tab).astype(np.int64)
    ix, iy, a, b = q[..., 0] >> 8, q[..., 1] >> 8, q[..., 0] & 255, q[..., 1] & 255

    def tap(yy, xx):
        inside = (xx >= 0) & (xx < ws) & (yy >= 0) & (yy < hs)
        val = src[np.clip(yy, 0, hs - 1), np.clip(xx, 0, ws - 1)].astype(np.int64)
        return np.where(inside[..., None], val, np.int64(border))

    wa, wb = (256 - a)[..., None], (256 - b)[..., None]
    a, b = a[..., None], b[..., None]
    acc = tap(iy, ix) * wa * wb + tap(iy, ix + 1) * a * wb + tap(iy + 1, ix) * wa * b + tap(iy + 1, ix + 1) * a * b + (1 << 15)
    assert acc.min() >= 0 and acc.max() < 1 << 31
    return (acc >> 16).astype(np.uint8)


def make_content(kind, h, w, seed=0):
    """uint8 [h,w,3]: "noise" or "extreme" (0 / 255 only)."""
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    return (np.stack([(x + y) % 2, (x // 3 + y // 2) % 2, (y // 5) % 2], -1) * 255).astype(np.uint8)
