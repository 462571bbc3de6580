"""Float64 oracle of the triangle rasteriser's rule (csrc/raster.hip), in numpy.

    vertex            c = (R_v^T (p - t_v)) * inv_s with render_twin.view_inverse; ok <=> near < c.z < far (strict);
                      u = fx * (c.x / c.z) + cx, v likewise (fx ... as the fp32 values the device gets);
                      in_guard <=> |u| <= G and |v| <= G, G = 16384; sx = floor(u * 256 + 0.5), sy likewise
    drawn face        indices in [0, V), vertices ok and in_guard, A = (bx-ax)(cy-ay) - (by-ay)(cx-ax) != 0 on (sx, sy);
                      cull "back" also drops A > 0 (clockwise on the screen, y down); no clipping of any kind
    coverage          b and c swapped when A < 0; E_i = (qx-px)(Y-py) - (qy-py)(X-px) for the edge p -> q from vertex i+1
                      to vertex i+2 at (X, Y) = (256 x, 256 y), python integers; covered <=> every E_i > 0, or E_i == 0 on
                      a top-left edge (dy < 0, or dy == 0 and dx > 0)
    depth             l_i = E_i / A, iz_i = 1 / z_i, w = (l_0 iz_0 + l_1 iz_1) + l_2 iz_2, z = 1 / w
    winner per pixel  smallest (z, face index)
    colour            m_i = l_i * iz_i * z; floor(((m_0 c_0 + m_1 c_1) + m_2 c_2) + 0.5) clamped to 0 ... 255

The device rounds every floating-point step to fp32, so the twin also marks what fp32 cannot decide.  A pixel is contested
when
    (a) for a face whose bounding box grown by one pixel holds it, the centre lies within two sub-pixel steps of the
        line of an edge, |E| <= 2 L + |dx| + |dy| (L the edge's length in steps), and not clearly outside the other two;
    (b) its two nearest covering faces differ by less than a relative Z_TIE in depth;
    (c) a face that covers it within those margins has a vertex whose depth is within a relative Z_EDGE of near or far,
        or whose |u| or |v| is within GUARD_EPS of G.
A vertex is an edge vertex when u * 256 + 0.5 or v * 256 + 0.5 lies within SNAP_EPS of an integer: fp32 may snap it one
step away.  The depth of an uncontested covered pixel is good to DEPTH_RTOL when its face has no edge vertex, else to
DEPTH_RTOL + (zmax / zmin - 1) * (2 / 256) / h_min (zmax, zmin the face's vertex depths, h_min its smallest altitude in
pixels): what a one-step move of a vertex can do to the interpolated depth.

check_against_twin states what a device image has to satisfy; fp32_emulation is the same rule in numpy float32, every
operation rounded as the device rounds it.
"""
import numpy as np

import render_twin as RT

S, G = 256, 16384.0
Z_TIE, Z_EDGE, GUARD_EPS, SNAP_EPS, DEPTH_RTOL = 1e-5, 1e-4, 1e-3, 0.02, 1e-5
MAX_CONTESTED = RT.MAX_CONTESTED
CULL = {"none": 0, "back": 1}


def vertex_stage(vertices, view, K, near, far, dtype=np.float64):
    """Per vertex: u, v, z in `dtype`, ok, in_guard, and the snapped (sx, sy) as int64 (0 where not ok and in_guard)."""
    f = dtype
    with np.errstate(all="ignore"):
        Rt, t, inv_s = RT.view_inverse(view, f)
        d = np.asarray(vertices, dtype=np.float32).reshape(-1, 3).astype(f) - t
        c = np.stack([((Rt[i, 0] * d[:, 0] + Rt[i, 1] * d[:, 1]) + Rt[i, 2] * d[:, 2]) * inv_s for i in range(3)], axis=1)
        fx, fy, cx, cy = (f(np.float32(k)) for k in K)
        z = c[:, 2]
        ok = (z > f(np.float32(near))) & (z < f(np.float32(far)))
        u, v = fx * (c[:, 0] / z) + cx, fy * (c[:, 1] / z) + cy
        guard = (np.abs(u) <= G) & (np.abs(v) <= G)
        a, b = u * f(S) + f(0.5), v * f(S) + f(0.5)
        use = ok & guard
        sx = np.floor(np.where(use, a, 0)).astype(np.int64)
        sy = np.floor(np.where(use, b, 0)).astype(np.int64)
    return dict(u=u, v=v, z=z, ok=ok, guard=guard, sx=sx, sy=sy, a=a, b=b)


def _oriented(vs, face, cull):
    """(rows in oriented order, A > 0) of a face, or None when it is not drawn."""
    V = vs["z"].shape[0]
    i = [int(k) for k in face]
    if any(k < 0 or k >= V for k in i) or not all(vs["ok"][k] and vs["guard"][k] for k in i):
        return None
    x, y = [int(vs["sx"][k]) for k in i], [int(vs["sy"][k]) for k in i]
    A = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
    if A == 0 or (cull and A > 0):
        return None
    return ([i[0], i[2], i[1]], -A) if A < 0 else (i, A)


def _edges(vs, rows, X, Y):
    """Per edge i (vertex i+1 -> vertex i+2): E at the pixel centres (X, Y) (int64 arrays in steps), top-left flag and
    the margin 2 L + |dx| + |dy| of condition (a)."""
    out = []
    for i in range(3):
        p, q = rows[(i + 1) % 3], rows[(i + 2) % 3]
        px, py, qx, qy = int(vs["sx"][p]), int(vs["sy"][p]), int(vs["sx"][q]), int(vs["sy"][q])
        dx, dy = qx - px, qy - py
        out.append((dx * (Y - py) - dy * (X - px), dy < 0 or (dy == 0 and dx > 0), 2.0 * float(np.hypot(dx, dy)) + abs(dx) + abs(dy)))
    return out


def _shade(E, A, z3, c3, f):
    """(z, colour value before the floor, both in dtype f) from the edge values E[3], the area and the vertex data."""
    with np.errstate(all="ignore"):
        l = [e.astype(f) / f(A) for e in E]
        iz = [f(1) / f(z) for z in z3]
        z = f(1) / ((l[0] * iz[0] + l[1] * iz[1]) + l[2] * iz[2])
        m = [l[i] * iz[i] * z for i in range(3)]
        val = np.stack([(m[0] * f(c3[0][ch]) + m[1] * f(c3[1][ch])) + m[2] * f(c3[2][ch]) for ch in range(3)], axis=-1)
    return z, val


def _box(vs, rows, size, grow):
    Hv, Wv = size
    xs, ys = [int(vs["sx"][k]) for k in rows], [int(vs["sy"][k]) for k in rows]
    x0, x1 = max(0, -((-min(xs)) // S) - grow), min(Wv - 1, max(xs) // S + grow)
    y0, y1 = max(0, -((-min(ys)) // S) - grow), min(Hv - 1, max(ys) // S + grow)
    return x0, x1, y0, y1


def raster_twin(vertices, colors, faces, view, K, size, near=1e-3, far=np.inf, cull="none", background=(0, 0, 0),
                dtype=np.float64):
    """vertices float32 [V,3], colors uint8 [V,3], faces int32 [F,3].  Returns a dict: rgb uint8 [Hv,Wv,3], value (the
    colour before the floor) [Hv,Wv,3], depth [Hv,Wv] (+inf: nothing), index int64 [Hv,Wv] (-1: nothing), covered and
    contested bool [Hv,Wv], and what check_against_twin needs per face."""
    Hv, Wv = size
    f = dtype
    colors, faces = np.asarray(colors, dtype=np.uint8).reshape(-1, 3), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    near, far = float(np.float32(near)), float(np.float32(far))
    vs = vertex_stage(vertices, view, K, near, far, f)
    with np.errstate(all="ignore"):
        z64, u64, v64 = (vs[k].astype(np.float64) for k in ("z", "u", "v"))
        z_edge = (np.abs(z64 - near) <= Z_EDGE * near) | (np.isfinite(far) & (np.abs(z64 - far) <= Z_EDGE * far))
        g_edge = (np.abs(np.abs(u64) - G) <= GUARD_EPS) | (np.abs(np.abs(v64) - G) <= GUARD_EPS)
        snap_edge = (np.abs(vs["a"] - np.round(vs["a"])) < SNAP_EPS) | (np.abs(vs["b"] - np.round(vs["b"])) < SNAP_EPS)
    # condition (c) looks at faces that fp32 may draw although float64 does not: their vertices count as drawable
    loose_vs = dict(vs)
    loose_vs["ok"], loose_vs["guard"] = vs["ok"] | (z_edge & (z64 > 0)), vs["guard"] | g_edge
    with np.errstate(all="ignore"):
        keep = loose_vs["ok"] & loose_vs["guard"]
        loose_vs["sx"] = np.floor(np.where(keep, vs["a"], 0)).astype(np.int64)
        loose_vs["sy"] = np.floor(np.where(keep, vs["b"], 0)).astype(np.int64)
    best = np.full((Hv, Wv), np.inf, dtype=f)
    second = np.full((Hv, Wv), np.inf, dtype=f)
    index = np.full((Hv, Wv), -1, dtype=np.int64)
    value = np.zeros((Hv, Wv, 3), dtype=f)
    contested = np.zeros((Hv, Wv), dtype=bool)
    tol = np.full(len(faces), DEPTH_RTOL)
    tol_moved = np.full(len(faces), DEPTH_RTOL)
    h_min = np.full(len(faces), np.inf)
    for n, face in enumerate(faces):
        i = [int(k) for k in face]
        if any(k < 0 or k >= len(z64) for k in i) or not (loose_vs["ok"][i] & loose_vs["guard"][i]).all():
            continue
        o, lo = _oriented(vs, face, CULL[cull]), _oriented(loose_vs, face, CULL[cull])
        if lo is None:
            if len(set(i)) == 3 and _oriented(loose_vs, face, 0) is None:
                # zero area after the snap although the vertices differ: fp32 may give it an area
                x0, x1, y0, y1 = _box(loose_vs, i, size, 1)
                if x1 >= x0 and y1 >= y0:
                    X, Y = np.meshgrid(np.arange(x0, x1 + 1, dtype=np.int64) * S, np.arange(y0, y1 + 1, dtype=np.int64) * S)
                    for E, _, m in _edges(loose_vs, i, X, Y):
                        contested[y0:y1 + 1, x0:x1 + 1] |= (np.abs(E) <= m) & (m > 0)
            continue
        shaky = o is None or bool((z_edge | g_edge)[i].any())              # condition (c)
        rows, A = lo
        src = loose_vs
        zs = z64[rows]
        L = [np.hypot(src["sx"][rows[(i + 1) % 3]] - src["sx"][rows[(i + 2) % 3]],
                      src["sy"][rows[(i + 1) % 3]] - src["sy"][rows[(i + 2) % 3]]) / S for i in range(3)]
        h_min[n] = (A / (S * S)) / max(L)
        tol_moved[n] = DEPTH_RTOL + (zs.max() / zs.min() - 1.0) * (2.0 / S) / h_min[n]
        tol[n] = tol_moved[n] if snap_edge[rows].any() else DEPTH_RTOL
        x0, x1, y0, y1 = _box(src, rows, size, 1)
        if x1 < x0 or y1 < y0:
            continue
        X, Y = np.meshgrid(np.arange(x0, x1 + 1, dtype=np.int64) * S, np.arange(y0, y1 + 1, dtype=np.int64) * S)
        ed = _edges(src, rows, X, Y)
        inside = np.ones(X.shape, dtype=bool)
        near_edge = np.zeros(X.shape, dtype=bool)
        loose = np.ones(X.shape, dtype=bool)
        for E, top_left, m in ed:
            inside &= (E > 0) | ((E == 0) & top_left)
            near_edge |= np.abs(E) <= m
            loose &= E > -m
        sub = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        contested[sub] |= (near_edge & loose) | (shaky & loose)
        if o is None:
            continue
        z, val = _shade([e[0] for e in ed], A, vs["z"][rows], colors[rows], f)
        win = inside & (z < best[sub])
        lose = inside & ~win
        second[sub] = np.where(win, best[sub], np.where(lose, np.minimum(second[sub], z), second[sub]))
        best[sub] = np.where(win, z, best[sub])
        index[sub] = np.where(win, n, index[sub])
        value[sub] = np.where(win[..., None], val, value[sub])
    with np.errstate(all="ignore"):
        b64, s64 = best.astype(np.float64), second.astype(np.float64)
        contested |= (s64 - b64) < Z_TIE * b64                               # inf - inf = NaN: False
    covered = index >= 0
    bg = np.asarray(background, dtype=np.uint8)
    rgb = np.where(covered[..., None], np.clip(np.floor(value + f(0.5)), 0, 255), bg).astype(np.uint8)
    return dict(rgb=rgb, value=value.astype(np.float64), depth=best, index=index, covered=covered, contested=contested,
                size=size, background=bg, tol=tol, tol_moved=tol_moved, h_min=h_min, vs=vs, loose_vs=loose_vs,
                colors=colors, faces=faces, cull=CULL[cull])


def contested_share(tw) -> float:
    """Contested pixels as a share of the covered pixels (the test's condition: at most 5 %)."""
    covered = int(tw["covered"].sum())
    return float((tw["contested"] & tw["covered"]).sum()) / covered if covered else 0.0


def face_at(tw, n, x, y):
    """Face n at pixel (x, y) as far as the twin can tell: (it covers the pixel within the margins of (a), float64 depth,
    float64 colour value), or (False, nan, None) for a face nothing can draw."""
    o = _oriented(tw["loose_vs"], tw["faces"][n], tw["cull"]) if 0 <= n < len(tw["faces"]) else None
    if o is None:
        return False, np.nan, None
    rows, A = o
    ed = _edges(tw["loose_vs"], rows, np.array([x * S], dtype=np.int64), np.array([y * S], dtype=np.int64))
    z, val = _shade([e[0] for e in ed], A, tw["vs"]["z"][rows].astype(np.float64), tw["colors"][rows], np.float64)
    return all(e[0][0] > -e[2] for e in ed), float(z[0]), val[0]


def check_against_twin(tw, rgb, depth, index, label=""):
    """The device image against the twin.  Uncontested pixels: exact index, depth within the face's bound, every colour
    channel within 1 of the float64 value, background / +inf / -1 where nothing is drawn.  Contested pixels: -1 or a
    face that covers the pixel within the margins, depth and colour consistent with that face.  A scene with more than
    MAX_CONTESTED contested pixels fails as untestable."""
    Hv, Wv = tw["size"]
    assert rgb.shape == (Hv, Wv, 3) and depth.shape == (Hv, Wv) and index.shape == (Hv, Wv)
    share = contested_share(tw)
    covered = int(tw["covered"].sum())
    print(f"{label}: covered {covered} of {Hv * Wv} pixels, contested {100 * share:.2f} % of covered")
    assert share <= MAX_CONTESTED, f"scene is untestable: {100 * share:.2f} % of the covered pixels are contested"
    free = ~tw["contested"]
    assert np.array_equal(index[free], tw["index"][free])
    hit = free & tw["covered"]
    assert np.isposinf(depth[free & ~hit]).all() and (rgb[free & ~hit] == tw["background"]).all()
    want = tw["depth"][hit].astype(np.float64)
    rel = np.abs(depth[hit].astype(np.float64) - want) / want
    bound = tw["tol"][tw["index"][hit]]
    plain = bound == DEPTH_RTOL
    print(f"{label}: max relative depth error {rel[plain].max() if plain.any() else 0.0:.3g} on {int(plain.sum())} uncontested "
          f"pixels of faces without an edge vertex, {rel.max() if rel.size else 0.0:.3g} on all {int(hit.sum())} "
          f"(largest per-face bound {bound.max() if bound.size else 0.0:.3g})")
    assert (rel <= bound).all()
    dc = np.abs(rgb[hit].astype(np.float64) - tw["value"][hit])
    print(f"{label}: max |channel - float64 value| {dc.max() if dc.size else 0.0:.3g}")
    assert (dc <= 1.0).all()
    for y, x in zip(*np.nonzero(tw["contested"])):
        n = int(index[y, x])
        if n == -1:
            assert np.isposinf(depth[y, x]) and (rgb[y, x] == tw["background"]).all()
            continue
        ok, z, val = face_at(tw, n, int(x), int(y))
        assert ok, f"pixel ({x}, {y}) holds face {n}, which does not cover it"
        assert abs(float(depth[y, x]) - z) <= tw["tol_moved"][n] * z, (x, y, n, float(depth[y, x]), z)
        assert (np.abs(rgb[y, x].astype(np.float64) - val) <= 1.0 + 2.0 / tw["h_min"][n]).all(), (x, y, n)
    return share


def face_bounds(vs, faces):
    """Per face, the bound on what a one-step move of a vertex can do to the interpolated depth, DEPTH_RTOL + (zmax /
    zmin - 1) * (2 / 256) / h_min, from a vertex_stage and faces whose vertices are all drawable."""
    F = np.asarray(faces, dtype=np.int64)
    x, y, z = vs["sx"][F].astype(np.float64) / S, vs["sy"][F].astype(np.float64) / S, vs["z"][F].astype(np.float64)
    area2 = np.abs((x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0]))
    longest = np.max([np.hypot(x[:, i] - x[:, (i + 1) % 3], y[:, i] - y[:, (i + 1) % 3]) for i in range(3)], axis=0)
    with np.errstate(all="ignore"):
        return DEPTH_RTOL + (z.max(axis=1) / z.min(axis=1) - 1.0) * (2.0 / S) / (area2 / longest)


def check_same_surface(ta, a, tb, b, label=""):
    """Images a and b (rgb, depth, index) of a mesh and of subdivide() of it, with their twins: the same pixels are
    covered, every part lies inside its face, and the depths agree.  It is one surface, but each mesh snaps its own
    vertices: the two bounds of a one-step vertex move add up."""
    hit = a[2] >= 0
    assert np.array_equal(hit, b[2] >= 0)
    assert np.array_equal(a[2][hit], b[2][hit] // 4)
    bound = ta["tol_moved"][a[2][hit]] + tb["tol_moved"][b[2][hit]]
    rel = np.abs(a[1][hit].astype(np.float64) - b[1][hit]) / a[1][hit]
    print(f"{label}: {int(hit.sum())} pixels, max relative depth difference {rel.max():.3g}, smallest bound {bound.min():.3g}")
    assert (rel <= bound).all()
    return int(hit.sum())


def fp32_emulation(vertices, colors, faces, view, K, size, **kw):
    """The rule in numpy float32: (rgb, float32 depth, index) shaped like the device's outputs."""
    tw = raster_twin(vertices, colors, faces, view, K, size, dtype=np.float32, **kw)
    return tw["rgb"], tw["depth"].astype(np.float32), tw["index"]
