"""Float64 oracle of the headless renderer's rule (csrc/render.hip), in numpy.

    candidate(k, n)  <=>  C32[k][n] / float32(N_k) > thr (fp32 divide, strict, NaN fails; thr None: no test) and the
                          world point p = s R X + t (oracle.sim3.sim3_act_mlx in float64) finite and within fp32 range
    view inverse          rows of R_v^T (quaternion formula, no normalisation), t_v, 1 / s_v: float64, rounded to fp32
    camera point          c = (R_v^T (p - t_v)) * inv_s
    kept             <=>  near < c.z < far (strict)
    pixel                 px = floor(fx * (c.x / c.z) + cx + 0.5), py likewise (fx ... as the fp32 values the device gets)
    footprint             point_size x point_size around (px, py), clipped to the image
    winner per pixel      smallest (c.z, k * N + n)

The device rounds every step to fp32, so the twin also marks what fp32 cannot decide:

    edge source       u + 0.5 or v + 0.5 within PIX_EPS = 1e-3 of an integer, z within a relative Z_EDGE = 1e-4 of near or
                      far, or a world coordinate within a factor 2 of fp32 overflow
    contested pixel   an edge source could land on it under either rounding, or its two nearest candidates differ by
                      less than a relative Z_TIE = 1e-5 in z

check_against_twin states what a device image has to satisfy; fp32_emulation is the same rule in numpy float32 (not the
device's bits: numpy does not promise the device's operation order inside sim3_act), used to try scenes on the CPU.
"""
import numpy as np

from oracle import sim3 as S

PIX_EPS, Z_EDGE, Z_TIE, DEPTH_RTOL = 1e-3, 1e-4, 1e-5, 1e-5
FLT_MAX = float(np.finfo(np.float32).max)


def colours(img, layout):
    """uint8 [K,N,3] of img: "f32" float32 [K,3,N] planes, "u8" uint8 [K,N,3]."""
    if layout == "u8":
        return img
    with np.errstate(all="ignore"):
        v = np.where(np.isnan(img), np.float32(0), img)
        col = np.floor(np.clip(v, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)
    return np.ascontiguousarray(col.transpose(0, 2, 1))


def view_inverse(T, dtype=np.float64):
    """(Rt [3,3], t [3], inv_s) of the view pose T (8 fp32 values): float64 arithmetic, rounded to fp32, returned in
    `dtype`."""
    T = np.asarray(T, dtype=np.float32).reshape(8).astype(np.float64)
    x, y, z, w = T[3:7]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    with np.errstate(all="ignore"):
        inv_s = np.float64(1.0) / T[7]
    return R.T.astype(np.float32).astype(dtype), T[:3].astype(np.float32).astype(dtype), np.float32(inv_s).astype(dtype)


def sources(sc, view, K, near, far, thr, dtype=np.float64):
    """Per source (flattened k * N + n): candidate flag (before the depth test), u, v, z in `dtype`, world point."""
    Kf, N = sc["X"].shape[:2]
    f = dtype
    with np.errstate(all="ignore"):
        avg = sc["C"].astype(np.float32) / sc["Nk"].astype(np.float32)[:, None]
        if dtype == np.float64:
            world = S.sim3_act_mlx(sc["T"].astype(np.float64)[:, None, :], sc["X"].astype(np.float64))
        else:
            world = S.sim3_act_mlx(sc["T"].astype(np.float32)[:, None, :], sc["X"].astype(np.float32)).astype(np.float32)
        cand = np.isfinite(world).all(axis=2) & (np.abs(world) <= FLT_MAX).all(axis=2)
        if thr is not None:
            cand &= avg > np.float32(thr)
        Rt, t, inv_s = view_inverse(view, f)
        d = world.reshape(-1, 3).astype(f) - t
        c = np.stack([((Rt[i, 0] * d[:, 0] + Rt[i, 1] * d[:, 1]) + Rt[i, 2] * d[:, 2]) * inv_s for i in range(3)], axis=1)
        fx, fy, cx, cy = (f(np.float32(v)) for v in K)
        z = c[:, 2]
        u = fx * (c[:, 0] / z) + cx
        v = fy * (c[:, 1] / z) + cy
    return cand.reshape(-1), u, v, z, world.reshape(-1, 3)


def _splat(pix_x, pix_y, z, idx, size, r):
    """Winner and runner-up per pixel of the given sources with footprint radius r: (key z [P], index [P], second z [P])."""
    Hv, Wv = size
    P = Hv * Wv
    pp, zz, ii = [], [], []
    for oy in range(-r, r + 1):
        for ox in range(-r, r + 1):
            x, y = pix_x + ox, pix_y + oy
            ok = (x >= 0) & (x < Wv) & (y >= 0) & (y < Hv)
            pp.append((y[ok] * Wv + x[ok]))
            zz.append(z[ok])
            ii.append(idx[ok])
    pp, zz, ii = np.concatenate(pp), np.concatenate(zz), np.concatenate(ii)
    order = np.lexsort((ii, zz, pp))
    pp, zz, ii = pp[order], zz[order], ii[order]
    first = np.ones(pp.size, dtype=bool)
    first[1:] = pp[1:] != pp[:-1]
    win_z = np.full(P, np.inf)
    win_i = np.full(P, -1, dtype=np.int64)
    sec_z = np.full(P, np.inf)
    win_z[pp[first]], win_i[pp[first]] = zz[first], ii[first]
    second = np.zeros(pp.size, dtype=bool)
    second[1:] = first[:-1] & ~first[1:]
    sec_z[pp[second]] = zz[second]
    return win_z, win_i, sec_z


def render_twin(sc, view, K, size, near=1e-3, far=np.inf, thr=1.5, point_size=1, background=(0, 0, 0), dtype=np.float64):
    """sc: dict X float32 [K,N,3], C float32 [K,N], Nk int [K], T float32 [K,8], img, layout.  Returns a dict:
    rgb uint8 [Hv,Wv,3], depth float64 [Hv,Wv] (+inf: nothing), index int64 [Hv,Wv] (-1: nothing), contested bool [Hv,Wv],
    and the per-source arrays (cand, edge, u, v, z, in_range) that may_land uses."""
    Hv, Wv = size
    r = point_size // 2
    near, far = float(np.float32(near)), float(np.float32(far))
    cand, u, v, z, world = sources(sc, view, K, near, far, thr, dtype)
    with np.errstate(all="ignore"):
        in_range = (z > near) & (z < far)
        half = dtype(0.5)                                               # the float32 emulation rounds u + 0.5 as the device does
        a, b = (u + half).astype(np.float64), (v + half).astype(np.float64)
        reach = np.isfinite(a) & np.isfinite(b) & (np.abs(a) < 1e9) & (np.abs(b) < 1e9)
        z_edge = (np.abs(z - near) <= Z_EDGE * near) | (np.isfinite(far) & (np.abs(z - far) <= Z_EDGE * far))
        pix_edge = (np.abs(a - np.round(a)) < PIX_EPS) | (np.abs(b - np.round(b)) < PIX_EPS)
        big = (np.abs(world) > FLT_MAX / 2).any(axis=1) & np.isfinite(world).all(axis=1)
    passes_conf = cand | big if thr is None else (cand | (big & (sc["C"].astype(np.float32) / sc["Nk"].astype(np.float32)[:, None]
                                                                  > np.float32(thr)).reshape(-1)))
    drawn = cand & in_range & reach                                      # what the float64 rule draws
    edge = passes_conf & reach & ((drawn & pix_edge) | z_edge | big)     # what fp32 may decide differently
    idx = np.arange(cand.size, dtype=np.int64)
    px = np.floor(np.where(reach, a, 0)).astype(np.int64)
    py = np.floor(np.where(reach, b, 0)).astype(np.int64)
    win_z, win_i, sec_z = _splat(px[drawn], py[drawn], z[drawn].astype(np.float64), idx[drawn], size, r)
    with np.errstate(all="ignore"):
        contested = (sec_z - win_z) < Z_TIE * win_z                      # inf - inf = NaN: False
    # every pixel an edge source could reach under either rounding
    e = np.nonzero(edge)[0]
    if e.size:
        x0, x1 = np.floor(a[e] - PIX_EPS).astype(np.int64) - r, np.floor(a[e] + PIX_EPS).astype(np.int64) + r
        y0, y1 = np.floor(b[e] - PIX_EPS).astype(np.int64) - r, np.floor(b[e] + PIX_EPS).astype(np.int64) + r
        for oy in range(2 * r + 2):
            for ox in range(2 * r + 2):
                x, y = x0 + ox, y0 + oy
                ok = (x <= x1) & (y <= y1) & (x >= 0) & (x < Wv) & (y >= 0) & (y < Hv)
                contested[y[ok] * Wv + x[ok]] = True
    col = colours(sc["img"], sc["layout"]).reshape(-1, 3)
    rgb = np.empty((Hv * Wv, 3), dtype=np.uint8)
    rgb[:] = np.asarray(background, dtype=np.uint8)
    hit = win_i >= 0
    rgb[hit] = col[win_i[hit]]
    return dict(rgb=rgb.reshape(Hv, Wv, 3), depth=win_z.reshape(Hv, Wv), index=win_i.reshape(Hv, Wv),
                contested=contested.reshape(Hv, Wv), covered=hit.reshape(Hv, Wv), col=col, r=r, size=size,
                background=np.asarray(background, dtype=np.uint8),
                src=dict(ok=passes_conf & reach, a=a, b=b, z=z.astype(np.float64), near=near, far=far))


def may_land(tw, index, pix):
    """For flat pixel numbers `pix` and source indices `index` (>= 0): could that source win that pixel as far as the
    twin can tell - it passes the tests that are exact, its depth is within Z_EDGE of the range and the pixel lies in
    its footprint under either rounding."""
    s, r, (Hv, Wv) = tw["src"], tw["r"], tw["size"]
    a, b, z = s["a"][index], s["b"][index], s["z"][index]
    x, y = pix % Wv, pix // Wv
    with np.errstate(all="ignore"):
        ok = s["ok"][index] & (z > s["near"] * (1 - Z_EDGE)) & (z < s["far"] * (1 + Z_EDGE) if np.isfinite(s["far"]) else np.isfinite(z))
        ok &= (x >= np.floor(a - PIX_EPS) - r) & (x <= np.floor(a + PIX_EPS) + r)
        ok &= (y >= np.floor(b - PIX_EPS) - r) & (y <= np.floor(b + PIX_EPS) + r)
    return ok


def contested_share(tw) -> float:
    """Contested pixels as a share of the covered pixels (the test's condition: at most 5 %)."""
    covered = int(tw["covered"].sum())
    return float((tw["contested"] & tw["covered"]).sum()) / covered if covered else 0.0


MAX_CONTESTED = 0.05


def check_against_twin(tw, rgb, depth, index, label=""):
    """The device image against the twin: exact index / colour and depth within DEPTH_RTOL on uncontested pixels, -1 or
    a listed candidate on contested ones.  A scene with more than MAX_CONTESTED contested pixels fails as untestable."""
    Hv, Wv = tw["size"]
    assert rgb.shape == (Hv, Wv, 3) and depth.shape == (Hv, Wv) and index.shape == (Hv, Wv)
    share = contested_share(tw)
    covered = int(tw["covered"].sum())
    print(f"{label}: covered {covered} of {Hv * Wv} pixels, contested {100 * share:.2f} % of covered")
    assert share <= MAX_CONTESTED, f"scene is untestable: {100 * share:.2f} % of the covered pixels are contested"
    free = ~tw["contested"]
    assert np.array_equal(index[free], tw["index"][free])
    assert np.array_equal(rgb[free], tw["rgb"][free])
    hit = free & (tw["index"] >= 0)
    assert np.isposinf(depth[free & ~hit]).all()
    rel = np.abs(depth[hit].astype(np.float64) - tw["depth"][hit]) / tw["depth"][hit]
    print(f"{label}: max relative depth error on {int(hit.sum())} uncontested covered pixels {rel.max() if rel.size else 0.0:.3g}")
    assert (rel <= DEPTH_RTOL).all()
    con = np.nonzero(tw["contested"].reshape(-1))[0]
    got = index.reshape(-1)[con]
    on = got >= 0
    assert (got[~on] == -1).all()
    assert may_land(tw, got[on], con[on]).all()
    # whatever won a contested pixel, the image is consistent with it
    flat_rgb, flat_d = rgb.reshape(-1, 3), depth.reshape(-1)
    assert np.array_equal(flat_rgb[con[on]], tw["col"][got[on]])
    zrel = np.abs(flat_d[con[on]].astype(np.float64) - tw["src"]["z"][got[on]]) / tw["src"]["z"][got[on]]
    assert (zrel <= DEPTH_RTOL).all()
    assert np.isposinf(flat_d[con[~on]]).all() and (flat_rgb[con[~on]] == tw["background"]).all()
    return share


def fp32_emulation(sc, view, K, size, **kw):
    """The rule in numpy float32: (rgb, float32 depth, index) shaped like the device's outputs."""
    tw = render_twin(sc, view, K, size, dtype=np.float32, **kw)
    return tw["rgb"], tw["depth"].astype(np.float32), tw["index"]
