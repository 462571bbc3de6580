"""The mesh-smooth rule of include/m3slam.h in numpy, written from the header's text and not from the kernel, and the
scenes the smooth tests share.  Every float64 operation is one numpy operation, so it is rounded on its own."""
import numpy as np

LAM, MU = 0.5, -0.53                                                            # Open3D's defaults


# ---- the rule --------------------------------------------------------------------------------------------------------
def valid_faces(faces, V):
    """(the faces whose three rows lie in [0, V), the number of the others)."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = ((faces >= 0) & (faces < V)).all(axis=1)
    return faces[ok], int((~ok).sum())


def edges(faces, V):
    """(edge_rows int32 [E,2] as (lo, hi) in lexicographic order, faces_of int32 [E], invalid faces)."""
    good, invalid = valid_faces(faces, V)
    pairs = np.concatenate([good[:, [0, 1]], good[:, [1, 2]], good[:, [2, 0]]], axis=0)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]                                   # two equal rows: no edge
    pairs = np.stack([pairs.min(axis=1), pairs.max(axis=1)], axis=1)
    if len(pairs) == 0:
        return np.zeros((0, 2), np.int32), np.zeros((0,), np.int32), invalid
    rows, faces_of = np.unique(pairs, axis=0, return_counts=True)               # unique sorts rows lexicographically
    return rows.astype(np.int32), faces_of.astype(np.int32), invalid


def adjacency(faces, V):
    """(off int32 [V + 1], nbr int32 [2 E]): row(v) = the other ends of the unique edges at v, ascending."""
    rows = edges(faces, V)[0].astype(np.int64)
    src = np.concatenate([rows[:, 0], rows[:, 1]])
    dst = np.concatenate([rows[:, 1], rows[:, 0]])
    order = np.lexsort((dst, src))                                              # by src, then by dst
    off = np.zeros(V + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(src, minlength=V))
    return off.astype(np.int32), dst[order].astype(np.int32)


def topology(faces, V):
    """What mesh_topology returns, as a dict of numpy arrays and ints."""
    rows, faces_of, invalid = edges(faces, V)
    off, _ = adjacency(faces, V)
    boundary = np.zeros(V, bool)
    boundary[rows[faces_of == 1].reshape(-1)] = True
    return dict(edges=len(rows), boundary_edges=int((faces_of == 1).sum()), nonmanifold_edges=int((faces_of > 2).sum()),
                invalid_faces=invalid, degree=np.diff(off).astype(np.int32), boundary=boundary, edge_rows=rows,
                edge_faces=faces_of)


def smooth_pass(p, off, nbr, pinned, w):
    """One pass with weight w (a Python float that is an fp32 value) on positions float32 [V,3]."""
    V = p.shape[0]
    off = off.astype(np.int64)
    degree = np.diff(off)
    finite = np.isfinite(p).all(axis=1)
    p64 = p.astype(np.float64)
    s = np.zeros((V, 3), np.float64)
    n = np.zeros(V, np.int64)
    for k in range(int(degree.max()) if V else 0):                              # the k-th neighbour of every row that has one
        rows = np.nonzero(degree > k)[0]
        j = nbr[off[rows] + k].astype(np.int64)
        fin = finite[j]
        rows, j = rows[fin], j[fin]
        s[rows] = s[rows] + p64[j]                                              # a row appears once: one add per row and step
        n[rows] += 1
    move = finite & ~pinned & (n > 0)
    out = p.copy()
    m = s[move] / n[move].astype(np.float64)[:, None]
    out[move] = (p64[move] + np.float64(w) * (m - p64[move])).astype(np.float32)
    return out


def smooth(vertices, faces, iterations=10, method="taubin", lam=LAM, mu=MU, fix_boundary=False, pinned=None):
    """vertices' float32 [V,3] of smooth_mesh with the same arguments."""
    assert method in ("laplacian", "taubin") and iterations >= 0
    p = np.ascontiguousarray(vertices, dtype=np.float32).copy()
    V = p.shape[0]
    off, nbr = adjacency(faces, V)
    pin = np.zeros(V, bool) if pinned is None else np.asarray(pinned, bool).copy()
    if fix_boundary:
        pin |= topology(faces, V)["boundary"]
    lam, mu = float(np.float32(lam)), float(np.float32(mu))                     # rounded to fp32 once
    with np.errstate(over="ignore", invalid="ignore"):
        for _ in range(iterations):
            p = smooth_pass(p, off, nbr, pin, lam)
            if method == "taubin":
                p = smooth_pass(p, off, nbr, pin, mu)
    return p


# ---- scenes: (vertices float32 [V,3], colors uint8 [V,3], faces int32 [F,3]) ---------------------------------------------
def _colors(V, seed):
    return np.random.default_rng(seed).integers(0, 256, (V, 3), dtype=np.uint8)


def grid_faces(w, h):
    """Two triangles per square of a w x h vertex grid (row v = y * w + x), the diagonal from (x, y) to (x + 1, y + 1)."""
    x, y = np.meshgrid(np.arange(w - 1), np.arange(h - 1))
    a = (y * w + x).reshape(-1)
    return np.concatenate([np.stack([a, a + 1, a + w + 1], axis=1), np.stack([a, a + w + 1, a + w], axis=1)]).astype(np.int32)


def shuffled(faces, seed):
    return np.ascontiguousarray(faces[np.random.default_rng(seed).permutation(len(faces))])


def jittered_grid(w=40, h=30, seed=5, offset=0.0, face_seed=11):
    """w x h vertices (1200: more than one workgroup, the last not full), spacing 0.01, jittered, face rows shuffled."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    v = np.stack([x.reshape(-1) * 0.01, y.reshape(-1) * 0.01, np.zeros(w * h)], axis=1)
    v = v + rng.normal(size=v.shape) * 0.002 + offset
    return v.astype(np.float32), _colors(w * h, seed), shuffled(grid_faces(w, h), face_seed)


def grid_rim(w=40, h=30):
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    return ((x == 0) | (x == w - 1) | (y == 0) | (y == h - 1)).reshape(-1)


def offset_grid():
    """The grid 1e6 away from the origin: a float32 sum of six neighbours would differ from the float64 one."""
    return jittered_grid(17, 19, seed=6, offset=1e6, face_seed=12)


def fan(rim=200, seed=7):
    """One hub (row 0) and `rim` vertices around it: degree 200, more than a wave."""
    rng = np.random.default_rng(seed)
    t = np.arange(rim) * (2.0 * np.pi / rim)
    v = np.concatenate([[[0.0, 0.0, 0.3]], np.stack([np.cos(t), np.sin(t), np.zeros(rim)], axis=1)])
    v = v + rng.normal(size=v.shape) * 0.01
    i = np.arange(rim)
    f = np.stack([np.zeros(rim, np.int64), 1 + i, 1 + (i + 1) % rim], axis=1).astype(np.int32)
    return v.astype(np.float32), _colors(rim + 1, seed), shuffled(f, seed)


def odd_faces(seed=8):
    """A 12 x 11 grid with a NaN and an infinite vertex in its middle, and behind it: three faces on one edge, a face
    given twice, the same face with the opposite winding, (a, a, b), (a, a, a), and an isolated vertex."""
    w, h = 12, 11
    v, _, f = jittered_grid(w, h, seed=seed, face_seed=seed)
    v[5 * w + 4, 1] = np.nan
    v[6 * w + 7, 0] = np.inf
    rng = np.random.default_rng(seed)
    extra = rng.normal(size=(9, 3)).astype(np.float32)                          # rows n ... n + 8; n + 8 is isolated
    n = w * h
    more = np.array([[n, n + 1, n + 2], [n, n + 1, n + 3], [n + 1, n, n + 4],   # three faces on the edge (n, n + 1)
                     [n + 5, n + 6, n + 7], [n + 5, n + 6, n + 7],               # a face twice
                     [n + 7, n + 6, n + 5],                                     # and with the opposite winding
                     [n + 2, n + 2, n + 3], [n + 4, n + 4, n + 4]], dtype=np.int32)
    v = np.concatenate([v, extra])
    return v, _colors(len(v), seed), shuffled(np.concatenate([f, more]), seed + 1)


ODD_NAN, ODD_INF = 5 * 12 + 4, 6 * 12 + 7


def icosphere(subdivisions=3):
    """The unit icosphere: 642 vertices and 1280 faces at three subdivisions."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, g = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return np.array(v).astype(np.float32), _colors(len(v), 9), np.array(f, dtype=np.int32)


def noisy_icosphere(seed):
    v, c, f = icosphere()
    return v + (np.random.default_rng(seed).normal(size=v.shape) * 0.02).astype(np.float32), c, f


def integer_lattice(n=9):
    """n x n vertices at (2 j, 2 i, 6), two triangles per square: every sum and every mean of the rule is exact."""
    j, i = np.meshgrid(np.arange(n), np.arange(n))
    v = np.stack([2.0 * j.reshape(-1), 2.0 * i.reshape(-1), np.full(n * n, 6.0)], axis=1).astype(np.float32)
    return v, _colors(n * n, 10), grid_faces(n, n)


SCENES = {"grid": jittered_grid, "fan": fan, "odd": odd_faces, "offset": offset_grid, "icosphere": icosphere,
          "lattice": integer_lattice}
# hubs on both sides of the row lengths at which the device sorts a row another way: one thread up to 32 entries, a
# wave in rounds of 64 beyond
SCENES.update({f"fan{n}": (lambda n=n: fan(n, seed=n)) for n in (32, 33, 64, 65)})
