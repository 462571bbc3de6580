"""Seeded meshes and views for the rasteriser tests (plain helper module: numpy only).

Every scene is a dict: vertices float32 [V,3], colors uint8 [V,3], faces int32 [F,3], view float32 [8], K, size, kw (the
near / far / cull / background arguments).  general() scenes are sheets whose cells are about 6 pixels or more on the
screen, so that the twin's contested share stays under its cap; exact() scenes make every fp32 step of the vertex stage
exact (identity pose, fx = fy = 64, principal point on the 1/256 grid, depths in {1, 2, 4}, x / z and y / z multiples of
2^-10), so the fp32 emulation of the twin is the device's answer bit for bit.
"""
import numpy as np

IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1, 1], dtype=np.float32)


def sheet(nx, ny, fn, x0, x1, y0, y1):
    """(vertices float32 [nx*ny,3], faces int32) of z = fn(x, y) on a grid, triangulated as collect_mesh does it:
    (a, c, b) and (b, c, d), counter-clockwise seen from a camera that looks along +z with y down."""
    X, Y = np.meshgrid(np.linspace(x0, x1, nx), np.linspace(y0, y1, ny))
    V = np.stack([X, Y, fn(X, Y)], axis=-1).reshape(-1, 3).astype(np.float32)
    F = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a = j * nx + i
            b, c, d = a + 1, a + nx, a + nx + 1
            F += [(a, c, b), (b, c, d)]
    return V, np.asarray(F, dtype=np.int32)


def subdivide(V, C, F):
    """Every face split into four at its edge midpoints (new vertices appended, one per face corner pair; not merged)."""
    V, C = [np.asarray(V, dtype=np.float64)], [np.asarray(C, dtype=np.float64)]
    out, n = [], len(V[0])
    for a, b, c in np.asarray(F):
        mid = [(a, b), (b, c), (c, a)]
        V.append(np.stack([(V[0][p] + V[0][q]) / 2 for p, q in mid]))
        C.append(np.stack([(C[0][p] + C[0][q]) / 2 for p, q in mid]))
        ab, bc, ca = n, n + 1, n + 2
        n += 3
        out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
    return np.concatenate(V).astype(np.float32), np.floor(np.concatenate(C)).astype(np.uint8), np.asarray(out, dtype=np.int32)


def _colours(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, 3)).astype(np.uint8)


def _two_sheets():
    V1, F1 = sheet(17, 13, lambda X, Y: 2.0 + 0.3 * np.sin(3 * X) * np.cos(2 * Y), -1.3, 1.3, -1.0, 1.0)
    V2, F2 = sheet(9, 7, lambda X, Y: 1.4 + 0.1 * X + 0.05 * Y, -0.5, 0.4, -0.4, 0.3)
    return np.concatenate([V1, V2]), np.concatenate([F1, F2 + len(V1)]).astype(np.int32)


def _pose(t, w, s):
    """Pose with translation t, rotation vector w (small angles: quaternion (w / 2, 1) normalised) and scale s."""
    q = np.concatenate([np.asarray(w, dtype=np.float64) / 2, [1.0]])
    return np.concatenate([t, q / np.linalg.norm(q), [s]]).astype(np.float32)


GENERAL = ("front", "oblique", "near_third", "partial", "mixed")
SIZE, KC = (96, 128), (110.0, 110.0, 63.5, 47.5)


def general(name):
    """A wavy 17 x 13 sheet at depth about 2 with a tilted 9 x 7 sheet in front at about 1.4; cells about 8 pixels wide."""
    V, F = _two_sheets()
    sc = dict(vertices=V, colors=_colours(len(V), 5), faces=F, view=_pose([0.1, -0.05, -0.2], [0.10, -0.16, 0.04], 1.1),
              K=KC, size=SIZE, kw=dict(near=0.5, background=(9, 8, 7)))
    if name == "oblique":
        sc["view"] = _pose([0.9, -0.1, -0.1], [0.05, -0.7, 0.03], 1.0)
    elif name == "near_third":
        import raster_twin as RW
        z = RW.vertex_stage(V, sc["view"], KC, 0.0, np.inf)["z"]
        sc["kw"]["near"] = float(np.float32(np.percentile(z, 100.0 / 3)))       # a third of the vertices behind near
    elif name == "partial":
        sc["K"] = (230.0, 228.0, 20.25, 70.5)                                   # the view sees one corner of the mesh
    elif name == "mixed":
        flip = np.random.default_rng(7).uniform(size=len(F)) < 0.5
        sc["faces"] = np.where(flip[:, None], F[:, [0, 2, 1]], F).astype(np.int32)
    elif name != "front":
        raise ValueError(name)
    return sc


def large_quad_behind_sheet():
    """One screen-filling quad (two faces, far beyond the walk threshold) behind the tilted sheet of small faces."""
    V2, F2 = sheet(9, 7, lambda X, Y: 1.4 + 0.1 * X + 0.05 * Y, -0.5, 0.4, -0.4, 0.3)
    quad = np.array([[-4, -3, 2.5], [4, -3, 2.75], [-4, 3, 3.0], [4, 3, 3.25]], dtype=np.float32)
    V = np.concatenate([quad, V2])
    F = np.concatenate([np.array([[0, 2, 1], [1, 2, 3]], dtype=np.int32), F2 + 4]).astype(np.int32)
    return dict(vertices=V, colors=_colours(len(V), 11), faces=F, view=_pose([0.02, 0.01, -0.1], [0.02, 0.03, -0.01], 1.0),
                K=KC, size=SIZE, kw=dict(near=0.5))


def planar_sheet():
    """A tilted plane on a 5 x 5 grid whose vertices have exact coordinates (multiples of 1/64), seen from the identity
    pose: cells of 9.5 to 12.2 pixels, so every face's bounding box holds more than 64 pixels and goes the wave's way,
    and every face of subdivide() of it at most 64 (box_pixels counts them)."""
    V, F = sheet(5, 5, lambda X, Y: 2.25 + 0.25 * X + 0.125 * Y, -0.75, 0.75, -0.75, 0.75)
    assert np.array_equal(V * 64, np.round(V * 64))
    return dict(vertices=V, colors=_colours(len(V), 13), faces=F, view=IDENTITY.copy(), K=(64.0, 64.0, 63.5, 47.5), size=SIZE,
                kw=dict(near=0.5))


def subdivided(sc):
    V, C, F = subdivide(sc["vertices"], sc["colors"], sc["faces"])
    return dict(sc, vertices=V, colors=C, faces=F)


def box_pixels(sc):
    """Pixels in the screen-clipped bounding box of every face of a scene whose vertices are all drawable."""
    import raster_twin as RW
    vs = RW.vertex_stage(sc["vertices"], sc["view"], sc["K"], sc["kw"].get("near", 1e-3), sc["kw"].get("far", np.inf))
    assert (vs["ok"] & vs["guard"]).all()
    return np.array([(lambda b: max(0, b[1] - b[0] + 1) * max(0, b[3] - b[2] + 1))(RW._box(vs, [int(k) for k in f], sc["size"], 0))
                     for f in sc["faces"]])


def single_face():
    """One face over the whole of a 256 x 256 view."""
    V = np.array([[-6, -6, 2.0], [14, -6, 3.0], [-6, 14, 2.5]], dtype=np.float32)
    return dict(vertices=V, colors=_colours(3, 17), faces=np.array([[0, 2, 1]], dtype=np.int32), view=IDENTITY.copy(),
                K=(100.0, 100.0, 127.5, 127.5), size=(256, 256), kw=dict(near=0.5))


def exact(size, offset, seed, shared):
    """Triangles on an 8-pixel grid that reaches past the view on every side, vertex depths drawn from {1, 2, 4}; offset 0
    puts every vertex on a pixel centre and shared edges through pixel centres, offset k / 256 moves the mesh off them.
    shared False: a triangle soup with one colour per face.  Every sixth face is drawn twice (equal depths over the
    same pixels: the smaller index wins; `originals` counts the faces before the repeats), and one large face of depth 4
    lies behind everything."""
    rng = np.random.default_rng(seed)
    Hv, Wv = size
    cx, cy = Wv // 2 - 0.5 + offset / 256.0, Hv // 2 - 0.5 + offset / 256.0
    nx, ny = Wv // 8 + 3, Hv // 8 + 3
    u = (8.0 * np.arange(nx) - 8.0 + (Wv // 2) % 8)[None, :].repeat(ny, 0) + offset / 256.0
    v = (8.0 * np.arange(ny) - 8.0 + (Hv // 2) % 8)[:, None].repeat(nx, 1) + offset / 256.0
    z = 2.0 ** rng.integers(0, 3, size=(ny, nx))
    P = np.stack([z * ((u - cx) / 64.0), z * ((v - cy) / 64.0), z], axis=-1).reshape(-1, 3)
    _, F = sheet(nx, ny, lambda X, Y: X, 0, 1, 0, 1)
    F = np.where((rng.uniform(size=len(F)) < 0.3)[:, None], F[:, [0, 2, 1]], F)          # both windings
    originals = len(F)
    F = np.concatenate([F, F[::6]])
    back = np.array([[-2.0 * Wv, -2.0 * Hv], [-2.0 * Wv, 3.0 * Hv], [3.0 * Wv, -2.0 * Hv]])            # u - cx, v - cy; counter-clockwise
    back = np.stack([4.0 * back[:, 0] / 64.0, 4.0 * back[:, 1] / 64.0, [4.0] * 3], axis=1)
    if shared:
        V, C = np.concatenate([P, back]), _colours(len(P) + 3, seed + 1)
        F = np.concatenate([F, [[len(P), len(P) + 1, len(P) + 2]]])
    else:
        V = np.concatenate([P[F.reshape(-1)], back])
        C = np.concatenate([_colours(len(F), seed + 1).repeat(3, axis=0), _colours(1, seed + 2).repeat(3, axis=0)])
        F = np.arange(len(V)).reshape(-1, 3)
    V32 = V.astype(np.float32)
    assert np.array_equal(V32.astype(np.float64), V) and np.array_equal(V[:, :2] / V[:, 2:] * 1024, np.round(V[:, :2] / V[:, 2:] * 1024))
    return dict(vertices=V32, colors=C, faces=F.astype(np.int32), view=IDENTITY.copy(), K=(64.0, 64.0, cx, cy), size=size,
                kw=dict(near=0.5, background=(1, 2, 3)), originals=originals)


EXACT = [((48, 64), 0, False), ((48, 64), 37, True), ((48, 64), 0, True), ((1, 1), 0, False), ((3, 5), 0, False), ((3, 5), 37, True)]


def odd_size():
    """The front scene in a 61 x 83 view: 5063 pixels, the scalar tail of clear and resolve."""
    return dict(general("front"), size=(61, 83), K=(110.0, 110.0, 41.0, 30.0))


def twin_scenes():
    """(label, scene) of every scene the GPU tests compare with the float64 twin."""
    for name in GENERAL:
        yield name, general(name)
    yield "large_quad", large_quad_behind_sheet()
    yield "single_face", single_face()
    yield "planar", planar_sheet()
    yield "odd_size", odd_size()
