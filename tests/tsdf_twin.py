"""The two rules of the volumetric fusion (csrc/tsdf.hip) in numpy, what fp32 cannot decide about
them, and the volumes their tests use.  Plain helper module: numpy only.

integrate(..., dtype) and extract(..., dtype) take the arithmetic's type as consistency_twin.twin does.  float64 is the
oracle.  float32 is an emulation in exactly the device's operation order: the device code is contraction-free IEEE
arithmetic on a voxel centre formed in the kernel (no act() whose inner order numpy would not promise), so the float32
emulation is expected to be the device's bits.

Integration rule.
Inputs: the keyframe tables (X float32 [K,N,3] in each keyframe's own camera frame, C float32 [K,N], img, poses
float32 [K,8], N_k), the common grid H x W (N = H * W), a pinhole (fx, fy, cx, cy) of that grid, thr (or none), z_min,
and a volume: origin fp32 [3], voxel size vs > 0, trunc > 0 and dims Dx, Dy, Dz, each in 2 ... 1024 with
Dx * Dy * Dz <= 2^30.
  observation plane   D[j][m] = X_j[m].z when point (j, m) passes the exporter's confidence test (C / N_j > thr: fp32
                      divide, strict, NaN fails; thr none: no test), that z is finite and z > z_min; otherwise NaN.
                      This is exactly step 1 of the consistency rule.
  voxel (iz, iy, ix)  centre p.x = origin.x + ((float)ix + 0.5f) * vs, likewise y and z.  It holds sum = 0.f, n = 0
                      and the colour sums r = g = b = 0, cn = 0 as uint32.
  for j = 0 .. K-1    in ascending order, every keyframe:
                      c = view_point(view_inverse(T_j), p) as in view_dev.h.  Skip unless c.z > z_min (strict, NaN
                      fails).
                      px = floorf((fx * (c.x / c.z) + cx) + 0.5f), py likewise.  Skip unless 0 <= px < W and
                      0 <= py < H, compared as floats before converting to int.
                      d = D[j][py * W + px].  Skip if d is NaN.
                      sdf = (d - c.z) * s_j, s_j the pose's scale in fp32 (camera units to world units).  Skip unless
                      sdf >= -trunc: the voxel is occluded in j.
                      t = fminf(sdf / trunc, 1.f); sum += t; n += 1.  A voxel far in front of the surface counts as
                      free space with t = 1: this carves away floating outliers.
                      If sdf <= trunc: add the colour of pixel (py, px) of keyframe j (the export's colour rule:
                      uint8 passed through, float (uint8)floorf(min(max(v, 0), 1) * 255.0f)) to r, g, b; cn += 1.
  outputs             tsdf float32 [Dz,Dy,Dx] = sum / (float)n, or 1.f when n == 0; weight int32 [Dz,Dy,Dx] = n;
                      color uint8 [Dz,Dy,Dx,3] = (2 * r + cn) / (2 * cn) in integer division per channel, or 0 when
                      cn == 0; colored uint8 [Dz,Dy,Dx] = (cn > 0), the bit the extraction's colour rule needs.
Every fp32 operation is separately rounded, and the divides are IEEE.

Extraction rule (naive surface nets).
Inputs: tsdf, weight, color, colored, origin, vs and min_weight >= 1.
  valid voxel         weight >= min_weight.       inside voxel: tsdf < 0 (strict: a value of 0 is outside).
  cell (z, y, x)      for z < Dz-1, y < Dy-1, x < Dx-1, with the 8 corner voxels (z+dz, y+dy, x+dx).  Active iff all 8
                      corners are valid and are neither all inside nor all outside.
  vertex              one per active cell, in ascending (z, y, x).  Walk the 12 cell edges - the 4 x-edges by
                      (dz,dy) = (0,0),(0,1),(1,0),(1,1); then the 4 y-edges by (dz,dx); then the 4 z-edges by (dy,dx)
                      - and add the crossing point of every edge whose ends differ in "inside" to acc = 0 (per
                      component, in that order).  An edge from corner a to b = a + e_d has tt = Fa / (Fa - Fb); its
                      crossing point is a's 0/1 offsets as floats, with tt along d.  local = acc / (float)count;
                      world.x = origin.x + (((float)x + 0.5f) + local.x) * vs, likewise y and z.  Colour per channel:
                      the rounded integer mean over the corners with colored set, (2 * sum + m) / (2 * m), or 0 when
                      there is none.
  faces               visit every grid edge from voxel (z, y, x) along d, d in the order x, y, z.  It yields faces when
                      its ends differ in "inside" and its four surrounding cells all exist and are active: cells
                      (z-1..z, y-1..y, x) for d = x, (z-1..z, y, x-1..x) for d = y, (z, y-1..y, x-1..x) for d = z.
                      With (u, v, d) right-handed - d=x: (y,z), d=y: (z,x), d=z: (x,y) - the cells at (du,dv) =
                      (-1,-1),(0,-1),(0,0),(-1,0) are q0..q3.  First end inside: (q0,q1,q2),(q0,q2,q3); otherwise
                      (q3,q2,q1),(q3,q1,q0).  Face normals then point to the free-space side.  Faces come in
                      ascending (z, y, x, d, triangle).
  outputs             vertices float32 [V,3], colors uint8 [V,3], faces int32 [F,3] (rows of the vertex arrays).

What fp32 cannot decide.  A pair (voxel, j) is contested when c.z lies within a relative Z_EDGE = 1e-4 of z_min; or
u + 0.5 or v + 0.5 lies within PIX_EPS = 1e-3 of an integer while the voxel is within one pixel of the image; or
|sdf + trunc| <= S_EDGE * trunc with S_EDGE = 1e-4; or (for the colour alone) |sdf - trunc| <= S_EDGE * trunc.  A voxel is
contested when any of its pairs is.  On uncontested voxels the float64 twin's weight and colour are the device's, and
the tsdf differs by at most tsdf_tolerance; on a contested voxel the weight lies within the number of its contested
pairs.

tsdf_tolerance = 2^-24 * (16 * M / trunc + 2 K), M the largest absolute coordinate among voxel centres, camera centres
and depths.  Derivation: 2^-24 * M bounds half an ulp of any intermediate of magnitude <= M.  The voxel centre takes 2
roundings (the product and the sum with the origin; ix + 0.5 is exact), the difference to the camera centre 1, c.z
3 products of a rotation entry (itself rounded: |r| <= 1, so another half ulp each, 3) with 2 sums and the product with
1 / s (rounded, 1, and 1 for the product): 13 half-ulp terms of magnitude <= M up to the scale factor, which the
product of the difference with s_j takes back.  d is an input; d - c.z, the product with s_j and its rounding of s_j
are 3 more: 16 terms, each divided by trunc on the way into t.  t itself (|t| <= 1) takes one rounding for the divide;
the running sum of K terms of magnitude <= K takes K roundings of at most 2^-24 * K, i.e. 2^-24 per term after the
divide by n; the final divide one more: at most 2 K * 2^-24 in all for K >= 1.  The formula is stated from this count,
never fitted to a device's output.
"""
import numpy as np

import consistency_twin as CT
import render_twin as RT

PIX_EPS, Z_EDGE, S_EDGE, MAX_CONTESTED = 1e-3, 1e-4, 1e-4, 0.05

# the volume of tests/test_gpu_fusion.py: odd dims, so every tail path runs
VOLUME = dict(origin=np.array([-2.0, -1.0, 1.9375], dtype=np.float32), vs=2.0 ** -5, trunc=2.0 ** -3, dims=(37, 41, 45))


def volume(dims, origin=VOLUME["origin"], vs=VOLUME["vs"], trunc=VOLUME["trunc"]):
    """dims = (Dz, Dy, Dx)."""
    return dict(origin=np.asarray(origin, dtype=np.float32), vs=float(np.float32(vs)), trunc=float(np.float32(trunc)),
                dims=tuple(int(d) for d in dims))


def bounds_of(vol):
    """The (lo, hi) bounds that fusion.volume_grid pads by trunc + vs and snaps back to exactly this volume (the origin is
    a multiple of vs and trunc is one too, as in VOLUME)."""
    o = vol["origin"].astype(np.float64)
    pad = vol["trunc"] + vol["vs"]
    Dz, Dy, Dx = vol["dims"]
    return o + pad, o + np.array([Dx, Dy, Dz]) * vol["vs"] - pad


def centres(vol, dtype=np.float64):
    """Voxel centres as three flat arrays x, y, z of Dz * Dy * Dx values (x fastest), in `dtype` in the device's order."""
    f = dtype
    o, vs, half = vol["origin"].astype(f), f(np.float32(vol["vs"])), f(0.5)
    Dz, Dy, Dx = vol["dims"]
    ax = [o[a] + (np.arange(n).astype(f) + half) * vs for a, n in ((0, Dx), (1, Dy), (2, Dz))]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return x.reshape(-1), y.reshape(-1), z.reshape(-1)


def pixel_colours(sc):
    """uint8 [K,N,3] by the export's colour rule."""
    img = sc["img"]
    if sc["layout"] == "u8":
        return img.reshape(sc["K"], sc["N"], 3)
    v = img.reshape(sc["K"], 3, sc["N"]).astype(np.float32)
    with np.errstate(all="ignore"):
        v = np.where(np.isnan(v), np.float32(0), np.minimum(np.maximum(v, np.float32(0)), np.float32(1)))
        return np.floor(v * np.float32(255)).astype(np.uint8).transpose(0, 2, 1)


def integrate(sc, pinhole, vol, thr=1.5, z_min=1e-3, dtype=np.float64):
    """sc as consistency_twin.twin takes it (K may be 0: X of shape [0,N,3]).  Returns a dict: tsdf float32, weight int32,
    color uint8 [..,3], colored uint8, pairs / cpairs int64 (contested pairs per voxel; colour-only ones) shaped
    [Dz,Dy,Dx], and sum (the running sum in `dtype`)."""
    f = dtype
    Kf, N = sc["X"].shape[:2]
    H, W = sc["H"], sc["W"]
    assert H * W == N
    Dz, Dy, Dx = vol["dims"]
    total = Dz * Dy * Dx
    zmin, trunc, one, half = f(np.float32(z_min)), f(np.float32(vol["trunc"])), f(1), f(0.5)
    fx, fy, cx, cy = (f(np.float32(v)) for v in pinhole)
    x, y, z = centres(vol, f)
    acc = np.zeros(total, dtype=f)
    n = np.zeros(total, dtype=np.int64)
    rgb = np.zeros((total, 3), dtype=np.int64)
    cn = np.zeros(total, dtype=np.int64)
    pairs = np.zeros(total, dtype=np.int64)
    cpairs = np.zeros(total, dtype=np.int64)
    with np.errstate(all="ignore"):
        if Kf:
            avg = sc["C"].astype(np.float32) / sc["Nk"].astype(np.float32)[:, None]
            passes = np.ones((Kf, N), dtype=bool) if thr is None else avg > np.float32(thr)
            z_own = sc["X"][..., 2].astype(np.float32)
            D = np.where(passes & np.isfinite(z_own) & (z_own > np.float32(z_min)), z_own, np.float32(np.nan)).astype(f)
            colours = pixel_colours(sc)
        for j in range(Kf):
            Rt, t, inv_s = RT.view_inverse(sc["T"][j], f)
            dx, dy, dz = x - t[0], y - t[1], z - t[2]
            c = [((Rt[i, 0] * dx + Rt[i, 1] * dy) + Rt[i, 2] * dz) * inv_s for i in range(3)]
            cz = c[2]
            front = cz > zmin
            a = (fx * (c[0] / cz) + cx) + half
            b = (fy * (c[1] / cz) + cy) + half
            pa, pb = np.floor(a), np.floor(b)
            inside = front & (pa >= 0) & (pa < W) & (pb >= 0) & (pb < H)
            pix = np.where(inside, pb * W + pa, 0).astype(np.int64)
            d = np.where(inside, D[j][pix], f(np.nan))
            seen = inside & ~np.isnan(d)
            sdf = (d - cz) * f(np.float32(sc["T"][j, 7]))
            used = seen & (sdf >= -trunc)
            tt = np.minimum(sdf / trunc, one)
            acc = np.where(used, acc + tt, acc)
            n += used
            col = used & (sdf <= trunc)
            rgb += np.where(col[:, None], colours[j][pix].astype(np.int64), 0)
            cn += col
            # what fp32 cannot decide
            z_edge = np.abs(cz - zmin) <= Z_EDGE * zmin
            maybe_front = cz > zmin * (1 - Z_EDGE)
            a64, b64 = a.astype(np.float64), b.astype(np.float64)
            near_image = np.isfinite(a64) & np.isfinite(b64) & (a64 > -1) & (a64 < W + 1) & (b64 > -1) & (b64 < H + 1)
            pix_edge = maybe_front & near_image & ((np.abs(a64 - np.round(a64)) < PIX_EPS) | (np.abs(b64 - np.round(b64)) < PIX_EPS))
            pairs += z_edge | pix_edge | (seen & (np.abs(sdf + trunc) <= S_EDGE * trunc))
            cpairs += seen & (np.abs(sdf - trunc) <= S_EDGE * trunc)
        tsdf = np.where(n > 0, acc / n.astype(f), one).astype(np.float32)
        color = np.where(cn[:, None] > 0, (2 * rgb + cn[:, None]) // np.maximum(2 * cn[:, None], 1), 0).astype(np.uint8)
    shape = (Dz, Dy, Dx)
    return dict(tsdf=tsdf.reshape(shape), weight=n.astype(np.int32).reshape(shape), color=color.reshape(shape + (3,)),
                colored=(cn > 0).astype(np.uint8).reshape(shape), pairs=pairs.reshape(shape), cpairs=cpairs.reshape(shape),
                sum=acc.reshape(shape))


def contested_share(tw) -> float:
    """Contested voxels as a share of the voxels some keyframe reaches (observed or contested): at most 5 % in a test."""
    con = (tw["pairs"] > 0) | (tw["cpairs"] > 0)
    reached = con | (tw["weight"] > 0)
    return float(con.sum()) / int(reached.sum()) if reached.any() else 0.0


def tsdf_tolerance(sc, vol) -> float:
    """The bound of the module docstring for this scene and volume."""
    x, y, z = centres(vol)
    M = max(np.abs(x).max(), np.abs(y).max(), np.abs(z).max())
    if sc["X"].shape[0]:
        zc = sc["X"][..., 2].astype(np.float64)
        M = max(M, float(np.abs(sc["T"][:, :3]).max()), float(np.abs(zc[np.isfinite(zc)]).max()))
    return 2.0 ** -24 * (16 * M / vol["trunc"] + 2 * max(1, sc["X"].shape[0]))


def check_integration(dev_out, tw64, tw32, sc, vol, label=""):
    """Device outputs (numpy: tsdf float32, weight int32, color uint8, colored uint8) against both twins, as the module
    docstring states.  Prints every figure before it asserts."""
    tsdf, weight, color, colored = dev_out
    tol = tsdf_tolerance(sc, vol)
    share = contested_share(tw64)
    free = (tw64["pairs"] == 0)
    cfree = free & (tw64["cpairs"] == 0)
    err = float(np.abs(tsdf.astype(np.float64) - tw64["tsdf"].astype(np.float64))[free].max()) if free.any() else 0.0
    emu = float(np.abs(tw32["tsdf"].astype(np.float64) - tw64["tsdf"].astype(np.float64))[free].max()) if free.any() else 0.0
    diff32 = int((tsdf.view(np.uint32) != tw32["tsdf"].view(np.uint32)).sum())
    print(f"{label}: observed {100 * float((tw64['weight'] > 0).mean()):.1f} %, weight 0..{int(tw64['weight'].max())}, contested "
          f"{100 * share:.2f} %, tol {tol:.3g}, |tsdf - f64| {err:.3g} (emulation {emu:.3g}), {diff32} tsdf words differ from the "
          f"f32 twin, {int((weight != tw32['weight']).sum())} weights, {int((color != tw32['color']).sum())} colour bytes")
    assert tol <= 1e-4
    assert share <= MAX_CONTESTED, f"volume is untestable: {100 * share:.2f} % of the reached voxels are contested"
    assert tsdf.dtype == np.float32 and weight.dtype == np.int32 and color.dtype == np.uint8 and colored.dtype == np.uint8
    # the float32 twin: the device's bits on every voxel
    assert tsdf.tobytes() == tw32["tsdf"].tobytes()
    assert np.array_equal(weight, tw32["weight"]) and np.array_equal(color, tw32["color"]) and np.array_equal(colored, tw32["colored"])
    # the float64 twin on uncontested voxels
    assert np.array_equal(weight[free], tw64["weight"][free])
    assert np.array_equal(color[cfree], tw64["color"][cfree]) and np.array_equal(colored[cfree], tw64["colored"][cfree])
    assert err <= tol
    con = ~free
    assert (np.abs(weight[con].astype(np.int64) - tw64["weight"][con]) <= tw64["pairs"][con]).all()
    return tol, err


# ---- extraction ------------------------------------------------------------------------------------------------------
_EDGE_OFFSETS = []                                                     # the 12 cell edges in the rule's order: (d, (dz, dy, dx) of a)
for _d in range(3):
    for _s in (0, 1):
        for _t in (0, 1):
            _EDGE_OFFSETS.append((_d, ((_s, _t, 0), (_s, 0, _t), (0, _s, _t))[_d]))
_UNIT = {0: (0, 0, 1), 1: (0, 1, 0), 2: (1, 0, 0)}                      # e_d as (dz, dy, dx) for d = x, y, z
_UV = {0: (1, 2), 1: (2, 0), 2: (0, 1)}                                 # (u, v) of d, right-handed


def _shift(a, dz, dy, dx):
    """b[z, y, x] = a[z + dz, y + dy, x + dx], False where that is outside."""
    b = np.zeros_like(a)
    Dz, Dy, Dx = a.shape
    src = tuple(slice(max(o, 0), n + min(o, 0)) for o, n in ((dz, Dz), (dy, Dy), (dx, Dx)))
    dst = tuple(slice(max(-o, 0), n + min(-o, 0)) for o, n in ((dz, Dz), (dy, Dy), (dx, Dx)))
    b[dst] = a[src]
    return b


def extract(tsdf, weight, color, colored, origin, vs, min_weight=1, dtype=np.float64):
    """(vertices [V,3] in `dtype`, colors uint8 [V,3], faces int32 [F,3]) of a volume by the extraction rule."""
    f = dtype
    F = np.asarray(tsdf, dtype=np.float32).astype(f)
    Dz, Dy, Dx = F.shape
    valid = np.asarray(weight) >= min_weight
    with np.errstate(all="ignore"):
        inside = F < 0
    allv = np.ones((Dz, Dy, Dx), dtype=bool)
    nin = np.zeros((Dz, Dy, Dx), dtype=np.int64)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                allv &= _shift(valid, dz, dy, dx)
                nin += _shift(inside, dz, dy, dx)
    active = allv & (nin > 0) & (nin < 8)
    active[Dz - 1:, :, :] = False                                        # the cell has to exist
    active[:, Dy - 1:, :] = False
    active[:, :, Dx - 1:] = False
    cz, cy, cx = np.nonzero(active)                                     # ascending (z, y, x)
    V = cz.size
    acc = [np.zeros(V, dtype=f) for _ in range(3)]                      # x, y, z
    count = np.zeros(V, dtype=np.int64)
    with np.errstate(all="ignore"):
        for d, (dz, dy, dx) in _EDGE_OFFSETS:
            ez, ey, ex = _UNIT[d]
            Fa, Fb = F[cz + dz, cy + dy, cx + dx], F[cz + dz + ez, cy + dy + ey, cx + dx + ex]
            cross = (Fa < 0) != (Fb < 0)
            tt = Fa / (Fa - Fb)
            point = [np.full(V, f(dx)), np.full(V, f(dy)), np.full(V, f(dz))]
            point[d] = tt
            for a in range(3):
                acc[a] = np.where(cross, acc[a] + point[a], acc[a])
            count += cross
        o, vsf, half = np.asarray(origin, dtype=np.float32).astype(f), f(np.float32(vs)), f(0.5)
        cnt = count.astype(f)
        vertices = np.stack([o[a] + ((idx.astype(f) + half) + acc[a] / cnt) * vsf for a, idx in ((0, cx), (1, cy), (2, cz))], axis=1)
    col = np.asarray(color).astype(np.int64)
    has = np.ones((Dz, Dy, Dx), dtype=bool) if colored is None else np.asarray(colored) != 0
    cs = np.zeros((V, 3), dtype=np.int64)
    m = np.zeros(V, dtype=np.int64)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                h = has[cz + dz, cy + dy, cx + dx]
                cs += np.where(h[:, None], col[cz + dz, cy + dy, cx + dx], 0)
                m += h
    colors = np.where(m[:, None] > 0, (2 * cs + m[:, None]) // np.maximum(2 * m[:, None], 1), 0).astype(np.uint8)
    remap = np.full((Dz, Dy, Dx), -1, dtype=np.int64)
    remap[cz, cy, cx] = np.arange(V)
    keys, quads = [], []
    for d in range(3):
        e = _UNIT[d]
        unit = [np.eye(3, dtype=np.int64)[2 - a] for a in range(3)]     # axis x, y, z as (dz, dy, dx)
        u, v = unit[_UV[d][0]], unit[_UV[d][1]]
        cells = [-u - v, -v, 0 * u, -u]                                 # q0..q3 relative to (z, y, x)
        ok = inside != _shift(inside, *e)
        ok &= _shift(np.ones_like(inside), *e)                          # the second end exists
        for q in cells:
            ok &= _shift(active, *q)
        z, y, x = np.nonzero(ok)
        keys.append(((z * Dy + y) * Dx + x) * 3 + d)
        q = [remap[z + c[0], y + c[1], x + c[2]] for c in cells]
        first = inside[z, y, x]
        t0 = np.where(first[:, None], np.stack([q[0], q[1], q[2]], axis=1), np.stack([q[3], q[2], q[1]], axis=1))
        t1 = np.where(first[:, None], np.stack([q[0], q[2], q[3]], axis=1), np.stack([q[3], q[1], q[0]], axis=1))
        quads.append(np.stack([t0, t1], axis=1).reshape(-1, 6))
    keys, quads = np.concatenate(keys), np.concatenate(quads)
    faces = quads[np.argsort(keys, kind="stable")].reshape(-1, 3).astype(np.int32)
    return vertices, colors, faces


def mesh_topology(faces):
    """(E, the largest and smallest number of faces an undirected edge belongs to) of a triangle list."""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    e.sort(axis=1)
    _, counts = np.unique(e[:, 0] * (int(faces.max()) + 1) + e[:, 1], return_counts=True)
    return counts.size, int(counts.max()), int(counts.min())


SPHERE_CENTRE, SPHERE_RADIUS = np.array([11.3, 12.1, 12.6]), 7.4         # x, y, z in world units (voxels of 1 from 0)


def sphere_volume(n=24, seed=3):
    """(tsdf float32, weight int32, color uint8, colored uint8) of clip((|p - c| - 7.4) / 4, -1, 1) on n^3 voxels with
    voxel centres p = index + 0.5 (origin 0, voxel size 1); all weights 1, random colours, a tenth of the voxels uncoloured."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    r = np.sqrt((x + 0.5 - SPHERE_CENTRE[0]) ** 2 + (y + 0.5 - SPHERE_CENTRE[1]) ** 2 + (z + 0.5 - SPHERE_CENTRE[2]) ** 2)
    tsdf = np.clip((r - SPHERE_RADIUS) / 4, -1, 1).astype(np.float32)
    colored = (rng.uniform(size=(n, n, n)) > 0.1).astype(np.uint8)
    color = rng.integers(0, 256, size=(n, n, n, 3)).astype(np.uint8)
    return tsdf, np.ones((n, n, n), dtype=np.int32), color, colored


SPHERE_ORIGIN, SPHERE_VS = np.zeros(3, dtype=np.float32), 1.0


def hand_case():
    """Two keyframes of 2 x 2 at the identity pose, pinhole (1, 1, 0.5, 0.5), depths 2 (keyframe 0) and 2.25 / 2 / 4 / 2
    (keyframe 1), whose pixel 3 fails the confidence test.  The volume is 2 x 2 x 2 voxels of 0.5 around the optical axis
    with centres at z = 1.75 and 2.25, trunc = 0.5: every voxel centre (+-0.25, +-0.25, z) projects to
    u + 0.5 = 1 +- 0.25 / z, well inside pixel 0 or 1 per axis.  Returns (scene, pinhole, volume, tsdf, weight, color) with
    the expected values written out."""
    pin = (1.0, 1.0, 0.5, 0.5)
    rays = np.array([[-0.5, -0.5, 1], [0.5, -0.5, 1], [-0.5, 0.5, 1], [0.5, 0.5, 1]])
    zs = np.array([[2.0, 2.0, 2.0, 2.0], [2.25, 2.0, 4.0, 2.0]])
    X = (rays[None] * zs[:, :, None]).astype(np.float32)
    C = np.full((2, 4), 2.0, dtype=np.float32)
    C[1, 3] = 1.0                                                       # below 1.5: no observation
    T = np.tile(np.array([0, 0, 0, 0, 0, 0, 1, 1], dtype=np.float32), (2, 1))
    img = np.zeros((2, 4, 3), dtype=np.uint8)
    img[0] = [[10, 20, 30], [40, 50, 60], [70, 80, 90], [100, 110, 120]]
    img[1] = [[11, 21, 31], [41, 51, 60], [71, 81, 91], [101, 111, 121]]
    sc = dict(X=X, C=C, Nk=np.ones(2, dtype=np.int32), T=T, img=img, layout="u8", K=2, N=4, H=2, W=2)
    vol = volume((2, 2, 2), origin=[-0.5, -0.5, 1.5], vs=0.5, trunc=0.5)
    # voxel (iz, iy, ix) sees pixel iy * 2 + ix of both keyframes; sdf = d - z, t = min(sdf / 0.5, 1)
    #   z = 1.75: keyframe 0 0.25 -> 0.5; keyframe 1: 0.5 -> 1, 0.25 -> 0.5, 2.25 -> 1 (free space, no colour), none
    #   z = 2.25: keyframe 0 -0.25 -> -0.5; keyframe 1: 0 -> 0, -0.25 -> -0.5, 1.75 -> 1 (no colour), none
    tsdf = np.array([[[0.75, 0.5], [0.75, 0.5]], [[-0.25, -0.5], [0.25, -0.5]]], dtype=np.float32)
    weight = np.array([[[2, 2], [2, 1]], [[2, 2], [2, 1]]], dtype=np.int32)
    near = np.array([[[10.5, 20.5, 30.5], [40.5, 50.5, 60]], [[70, 80, 90], [100, 110, 120]]])   # means before rounding
    color = np.floor(near + 0.5).astype(np.uint8)                       # (2 r + cn) / (2 cn): halves round up
    color = np.stack([color, color])                                    # both z layers see the same pixels
    return sc, pin, vol, tsdf, weight, color


def shared_cases():
    """(label, scene, pinhole) of the three shared scenes, u8 and f32 layouts alternating as in test_gpu_consistency."""
    for K, H, W, seed in CT.SHARED:
        for layout in ("u8", "f32"):
            yield f"{K}x{H}x{W} {layout}", CT.shared_scene(K, H, W, seed, layout=layout), CT.shared_pinhole(H, W)
