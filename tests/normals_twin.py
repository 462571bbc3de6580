"""numpy twin of the vertex-normal and shading rules of include/m3slam.h (csrc/mesh_normals.hip, mast3r_slam/normals.py),
and the meshes the tests use (plain helper module: numpy only).

Two twins of the normals.  vertex_normals restates the rule operation by operation in float32 - face normal, threshold,
unit normal scaled by 2^24 and rounded to int64, the sums through np.add.at, the float64 finish - and is what the device
must give byte for byte.  vertex_normals64 is the same equal-weight rule in float64 without the quantisation; the gap
between the two is the error of the rule itself (tests/test_normals_host.py measures it).  shade is the shading rule,
in float32 (the device's bytes) or float64."""
import numpy as np

import raster_scenes as RS

MIN_LEN2 = 2.0 ** -80
SCALE = 16777216.0


# ---- the rule --------------------------------------------------------------------------------------------------------
def valid_faces(faces, V):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(axis=1)


def _cross(e1, e2):
    """Each component p * q - r * s: three separately rounded operations in the arrays' own type."""
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)


def face_contributions(vertices, faces):
    """(rows int64 [M,3], q int64 [M,3]) of the faces that contribute, in face order: float32 throughout."""
    P = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = f[valid_faces(f, len(P))]
    with np.errstate(all="ignore"):
        a, b, c = P[f[:, 0]], P[f[:, 1]], P[f[:, 2]]
        n = _cross(b - a, c - a)
        len2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        assert n.dtype == np.float32 and len2.dtype == np.float32
        ok = np.isfinite(len2) & (len2 >= np.float32(MIN_LEN2))
        n, length = n[ok], np.sqrt(len2[ok])
        u = n / length[:, None]
        q = np.rint(u * np.float32(SCALE))
    assert q.dtype == np.float32
    return f[ok], q.astype(np.int64)


def vertex_sums(vertices, faces):
    """int64 [V,3]: the sums the face pass leaves."""
    V = np.asarray(vertices).reshape(-1, 3).shape[0]
    rows, q = face_contributions(vertices, faces)
    sums = np.zeros((V, 3), dtype=np.int64)
    for i in range(3):
        np.add.at(sums, rows[:, i], q)
    return sums


def vertex_normals(vertices, faces):
    """float32 [V,3]: the rule, with the device's operation order."""
    s = vertex_sums(vertices, faces).astype(np.float64)
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    L = np.sqrt((x * x + y * y) + z * z)
    with np.errstate(all="ignore"):
        n = (s / L[:, None]).astype(np.float32)
    n[L == 0] = 0
    return n


def vertex_normals64(vertices, faces):
    """float64 [V,3]: unit face normals with equal weights in float64, no quantisation.  The same faces are left out
    (the threshold is applied to the float64 squared length)."""
    P = np.asarray(vertices, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = f[valid_faces(f, len(P))]
    with np.errstate(all="ignore"):
        n = _cross(P[f[:, 1]] - P[f[:, 0]], P[f[:, 2]] - P[f[:, 0]])
        len2 = (n * n).sum(axis=1)
        ok = np.isfinite(len2) & (len2 >= MIN_LEN2)
        u = n[ok] / np.sqrt(len2[ok])[:, None]
    s = np.zeros((len(P), 3))
    for i in range(3):
        np.add.at(s, f[ok][:, i], u)
    L = np.sqrt((s * s).sum(axis=1))
    with np.errstate(all="ignore"):
        out = s / L[:, None]
    out[L == 0] = 0
    return out


def _levels(x):
    """clamp(x, 0, 255) as fminf(fmaxf(x, 0), 255) and the conversion to uint8: a NaN gives 0."""
    with np.errstate(all="ignore"):
        return np.where(np.isnan(x), 0, np.clip(x, 0, 255)).astype(np.uint8)


def shade(vertices, normals, colors=None, eye=None, light=None, ambient=0.25, two_sided=True, mode="lambert",
          albedo=(200, 200, 200), dtype=np.float32):
    """uint8 [V,3]: the shading rule in `dtype` (float32: the device's operation order and bytes).  eye: the translation
    of the view pose (the headlight); light: a constant direction towards the light instead."""
    t = dtype
    P, N = np.asarray(vertices, dtype=np.float32).astype(t).reshape(-1, 3), np.asarray(normals, dtype=np.float32).astype(t).reshape(-1, 3)
    with np.errstate(all="ignore"):
        if mode == "normals":
            return _levels(np.floor((N * t(0.5) + t(0.5)) * t(255) + t(0.5)))
        assert mode == "lambert" and (eye is None) != (light is None)
        if light is None:
            l = np.asarray(eye, dtype=np.float32).astype(t).reshape(1, 3) - P
        else:
            l = np.broadcast_to(np.asarray(light, dtype=np.float32).astype(t).reshape(1, 3), P.shape)
        dot = (N[:, 0] * l[:, 0] + N[:, 1] * l[:, 1]) + N[:, 2] * l[:, 2]
        d = dot / np.sqrt((l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1]) + l[:, 2] * l[:, 2])
        if two_sided:
            d = np.abs(d)
        d = np.where(d > 0, np.minimum(d, t(1)), t(0)).astype(t)
        a = t(np.float32(ambient))
        I = a + (t(1) - a) * d
        C = (np.broadcast_to(np.asarray(albedo, dtype=np.uint8), P.shape) if colors is None
             else np.asarray(colors, dtype=np.uint8).reshape(-1, 3)).astype(t)
        x = np.floor(C * I[:, None] + t(0.5))
        assert x.dtype == t
        return _levels(x)


# ---- meshes ----------------------------------------------------------------------------------------------------------
def wavy(X, Y):
    return 2.0 + 0.3 * np.sin(3 * X) * np.cos(2 * Y)


def sheet(nx, ny, fn=wavy):
    """(vertices, faces) of raster_scenes.sheet over [-1.3, 1.3] x [-1, 1]: nx * ny vertices, 2 (nx - 1)(ny - 1) faces."""
    return RS.sheet(nx, ny, fn, -1.3, 1.3, -1.0, 1.0)


def two_sheets():
    sc = RS.general("front")
    return sc["vertices"], sc["faces"]


def fan(n=4096):
    """Row 0 is a hub shared by n faces (0, i, i + 1) over a rim of n + 1 vertices that rises and falls."""
    a = np.linspace(0.0, 2 * np.pi, n + 1)
    rim = np.stack([np.cos(a), np.sin(a), 0.2 * np.sin(5 * a)], axis=1)
    V = np.concatenate([[[0.0, 0.0, 0.3]], rim]).astype(np.float32)
    i = np.arange(1, n + 1)
    return V, np.stack([np.zeros(n, dtype=np.int64), i, i + 1], axis=1).astype(np.int32)


def sphere(levels=3):
    """A closed octahedron, every face split into four `levels` times with shared midpoints, pushed onto the unit sphere;
    faces counter-clockwise seen from outside, so normals point outwards."""
    V = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    F = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    V = [np.asarray(v, dtype=np.float64) for v in V]
    for _ in range(levels):
        mids, out = {}, []

        def mid(p, q):
            key = (min(p, q), max(p, q))
            if key not in mids:
                m = V[p] + V[q]
                V.append(m / np.linalg.norm(m))
                mids[key] = len(V) - 1
            return mids[key]

        for a, b, c in F:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        F = out
    return np.asarray(V, dtype=np.float32), np.asarray(F, dtype=np.int32)


def cube_with_centres():
    """The 8 corners of [-1, 1]^3 (rows 0 ... 7) and the 6 face centres (rows 8 ... 13, in the order +x -x +y -y +z -z), every
    face a fan of four triangles around its centre, counter-clockwise seen from outside."""
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64)
    V, F = list(corners), []
    for axis in range(3):
        for sign in (1, -1):
            n = np.zeros(3)
            n[axis] = sign
            ring = [i for i in range(8) if corners[i][axis] == sign]
            u, w = np.eye(3)[(axis + 1) % 3], np.eye(3)[(axis + 2) % 3]             # u x w = +axis
            ring.sort(key=lambda i: np.arctan2(corners[i] @ w, corners[i] @ u) * sign)
            V.append(n)
            centre = len(V) - 1
            F += [(centre, ring[k], ring[(k + 1) % 4]) for k in range(4)]
    return np.asarray(V, dtype=np.float32), np.asarray(F, dtype=np.int32)


def degenerate():
    """(vertices, faces, zero): a small sheet, then one face of every kind that contributes nothing, each on vertices of
    its own; zero = the rows whose normal must be (0, 0, 0).  Two faces of the sheet are also named by bad faces that
    share their vertices, and two opposite faces on three more vertices cancel exactly."""
    P, F = sheet(5, 4)
    n0 = len(P)
    extra = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2],                         # n0 + 0 ... 2: collinear
                      [np.nan, 0, 0], [0, 1, 0], [1, 0, 0],                      # + 3 ... 5: a NaN vertex
                      [np.inf, 0, 0], [0, 1, 0], [1, 0, 0],                      # + 6 ... 8: an infinite vertex
                      [0, 0, 0], [1e-25, 0, 0], [0, 1, 0],                       # + 9 ... 11: |e1 x e2|^2 = 1e-50 < 2^-80
                      [0, 0, 5], [1, 0, 5], [0, 1, 5],                           # + 12 ... 14: two opposite faces
                      [7, 7, 7], [8, 8, 8]], dtype=np.float32)                   # + 15, 16: unreferenced
    V = len(P) + len(extra)
    bad = [(0, 0, 1), (2, 3, 3),                                                 # a repeated index, on rows of the sheet
           (n0, n0 + 1, n0 + 2), (n0 + 3, n0 + 4, n0 + 5), (n0 + 6, n0 + 7, n0 + 8), (n0 + 9, n0 + 10, n0 + 11),
           (-1, 0, 1), (0, V, 1), (0, 1, -2 ** 31), (2 ** 31 - 1, 1, 2),          # outside [0, V), with rows of the sheet
           (n0 + 12, n0 + 13, n0 + 14), (n0 + 12, n0 + 14, n0 + 13)]
    faces = np.concatenate([F[:7], np.asarray(bad, dtype=np.int64), F[7:]]).astype(np.int32)
    return np.concatenate([P, extra]), faces, np.arange(n0, V)


def permuted(faces, seed=0):
    return np.ascontiguousarray(faces[np.random.default_rng(seed).permutation(len(faces))])


# ---- reading back what export.save_ply_mesh_normals wrote ----------------------------------------------------------
PLY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"),
                      ("green", "u1"), ("blue", "u1")])
FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
HEADER = ["property float x", "property float y", "property float z", "property float nx", "property float ny",
          "property float nz", "property uchar red", "property uchar green", "property uchar blue"]


def read_ply_mesh_normals(path):
    """(vertices, normals, colors, faces) of a file save_ply_mesh_normals wrote, binary or ASCII."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines()
    v, f = int(lines[2].split()[-1]), int(lines[12].split()[-1])
    assert lines[0] == "ply" and lines[2] == f"element vertex {v}" and lines[3:12] == HEADER
    assert lines[12:] == [f"element face {f}", "property list uchar int vertex_indices", "end_header"]
    if lines[1] == "format binary_little_endian 1.0":
        assert len(raw) == end + 27 * v + 13 * f
        body = np.frombuffer(raw, dtype=PLY_DTYPE, count=v, offset=end)
        tri = np.frombuffer(raw, dtype=FACE_DTYPE, count=f, offset=end + 27 * v)
        assert (tri["n"] == 3).all()
        cols = lambda *names: np.stack([body[n] for n in names], axis=1).reshape(v, 3)
        return cols("x", "y", "z"), cols("nx", "ny", "nz"), cols("red", "green", "blue"), tri["v"].reshape(f, 3)
    assert lines[1] == "format ascii 1.0"
    rows = raw[end:].decode("ascii").splitlines()
    assert len(rows) == v + f
    body = np.array([r.split() for r in rows[:v]], dtype=np.float64).reshape(v, 9)
    tri = np.array([r.split() for r in rows[v:]], dtype=np.int64).reshape(f, 4)
    assert (tri[:, 0] == 3).all()
    return body[:, :3], body[:, 3:6], body[:, 6:].astype(np.uint8), tri[:, 1:].astype(np.int32)
