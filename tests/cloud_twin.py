"""A numpy restatement of the point-cloud neighbourhood rule of include/m3slam.h (section "point cloud"), written from
that text: counts and moments as the device must give them byte for byte, the radius filter's selection, and the exact
covariance the normals are judged against.  Candidate pairs come from a k-d tree at a slightly larger radius; the
membership test and the sums follow the rule literally, in float64 and integers.  Every scene has at most about 4000
points: the per-point loop is the slow part."""
from fractions import Fraction

import numpy as np
from scipy.spatial import cKDTree


def radius32(radius):
    """(r, scale): the radius as the float32 value the device gets, and 2^20 / r in float64."""
    r = float(np.float32(radius))
    return r, 2.0 ** 20 / r


def cells(points, radius):
    """floor((double)p / h), h = r (1 + 2^-10), float64 [M,3]; NaN rows for points that are not finite."""
    r, _ = radius32(radius)
    h = r * (1.0 + 2.0 ** -10)
    with np.errstate(invalid="ignore"):
        return np.floor(points.astype(np.float64) / h)


def neighbors(points, radius):
    """dict(count int32 [M], moments int64 [M,9], out_of_range int, sets: the neighbour rows of every point)."""
    points = np.ascontiguousarray(points, dtype=np.float32)
    M = len(points)
    r, scale = radius32(radius)
    r2 = r * r
    P = points.astype(np.float64)
    finite = np.isfinite(points).all(axis=1)
    with np.errstate(invalid="ignore"):
        far = finite & ~(np.abs(cells(points, radius)) < 2.0 ** 20).all(axis=1)
    valid = finite & ~far
    rows = np.flatnonzero(valid)
    count = np.zeros(M, np.int32)
    moments = np.zeros((M, 9), np.int64)
    sets = [np.zeros(0, np.int64) for _ in range(M)]
    if len(rows):
        tree = cKDTree(P[rows])
        cand = tree.query_ball_point(P[rows], r * 1.001 + 1e-12)
        for a, i in enumerate(rows):
            j = rows[np.asarray(cand[a], dtype=np.int64)]
            d = P[j] - P[i]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            j = np.sort(j[d2 <= r2])                                            # inclusive
            q = np.rint((P[j] - P[i]) * scale).astype(np.int64)                 # round half to even
            sets[i] = j
            count[i] = len(j)
            moments[i, :3] = q.sum(axis=0)
            moments[i, 3:] = [(q[:, a_] * q[:, b_]).sum() for a_, b_ in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return dict(count=count, moments=moments, out_of_range=int(far.sum()), sets=sets)


def brute_counts(points, radius):
    """count by the O(M^2) float64 distance matrix: no tree, no cells."""
    r, _ = radius32(radius)
    P = np.asarray(points, np.float32).astype(np.float64)
    finite = np.isfinite(P).all(axis=1)
    with np.errstate(invalid="ignore"):
        d = P[None, :, :] - P[:, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        inside = (d2 <= r * r) & finite[None, :] & finite[:, None]
    return inside.sum(axis=1).astype(np.int32)


def covariance(count, moments):
    """C float64 [M,3,3] = (n S2 - S1 S1^T) / n^2, every entry the correctly rounded value of the exact rational; zeros
    where count is 0."""
    C = np.zeros((len(count), 3, 3))
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    for i, (n, m) in enumerate(zip(count.tolist(), moments.tolist())):
        if n == 0:
            continue
        for k, (a, b) in enumerate(pairs):
            C[i, a, b] = C[i, b, a] = float(Fraction(n * m[3 + k] - m[a] * m[b], n * n))
    return C


def judged(count, moments, min_points=3):
    """Rows that must carry a normal: count >= min_points and a covariance with a non-zero trace (exact)."""
    out = np.zeros(len(count), bool)
    for i, (n, m) in enumerate(zip(count.tolist(), moments.tolist())):
        out[i] = n >= min_points and sum(n * m[k] - m[a] * m[a] for k, a in ((3, 0), (6, 1), (8, 2))) != 0
    return out


def kept_rows(points, radius, min_neighbors, count=None):
    """Rows the radius filter keeps, ascending: finite points with at least min_neighbors other points within r."""
    count = neighbors(points, radius)["count"] if count is None else count
    return np.flatnonzero(count.astype(np.int64) - 1 >= min_neighbors).astype(np.int64)


# ---- scenes: (points float32 [M,3], radius) ---------------------------------------------------------------------------
def plane(noise=0.002, seed=0):
    g = np.random.default_rng(seed)
    p = np.concatenate([g.random((3000, 2)), noise * g.normal(size=(3000, 1))], axis=1)
    return p.astype(np.float32), 0.05


def flat_plane():
    return plane(noise=0.0)


SPHERE_CENTRE = np.array([3.0, -2.0, 7.0])


def sphere(seed=1):
    g = np.random.default_rng(seed)
    u = g.normal(size=(3000, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (SPHERE_CENTRE + 0.5 * u).astype(np.float32), 0.06


LATTICE_SIDE = 9


def _lattice_points():
    k = np.arange(LATTICE_SIDE) - LATTICE_SIDE // 2
    g = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64) / 8.0
    r2 = float(np.float32(0.125 * np.sqrt(2.0)))
    near = lambda v: np.round(v * 8.0) / 8.0                                    # the lattice point nearest a coordinate
    shifts = [np.zeros(3),
              np.array([1024 * 0.125, 2048 * 0.125, -1024 * 0.125]),            # crosses 128, 256 and -128
              np.array([near(1024 * r2), near(-2048 * r2), near(2048 * r2)])]   # crosses 1024 r and 2048 r of the other radius
    return np.concatenate([g + s for s in shifts]).astype(np.float32)


def lattice():
    return _lattice_points(), 0.125


def lattice_diagonal():
    return _lattice_points(), float(np.float32(0.125 * np.sqrt(2.0)))


def lattice_interior():
    """Rows of the lattice scenes whose six axis neighbours exist."""
    k = np.arange(LATTICE_SIDE)
    g = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)
    one = ((g > 0) & (g < LATTICE_SIDE - 1)).all(axis=1)
    return np.concatenate([one, one, one])


def ball(seed=2):
    r = 0.1
    g = np.random.default_rng(seed)
    u = g.normal(size=(2000, 3))
    u *= (0.3 * r * g.random((2000, 1)) ** (1.0 / 3.0)) / np.linalg.norm(u, axis=1, keepdims=True)
    return (np.array([1.0, 2.0, 3.0]) + u).astype(np.float32), r


N_ISOLATED, N_DUPLICATES = 50, 20


def floaters(seed=3):
    """plane, then 50 isolated points, 20 exact duplicates of plane rows and a NaN, a +inf and a -inf row, shuffled.
    Returns (points, radius); floaters_rows() names the rows."""
    p, r = plane()
    g = np.random.default_rng(seed)
    k = np.arange(N_ISOLATED)
    iso = np.stack([0.5 * (k % 8), 0.5 * (k // 8), 1.0 + 0.01 * k], axis=1)     # at least 0.5 from each other and the plane
    dup = p[g.choice(len(p), N_DUPLICATES, replace=False)]
    bad = np.array([[np.nan, 0.5, 0.0], [0.5, np.inf, 0.0], [0.5, 0.5, -np.inf]])
    allp = np.concatenate([p, iso, dup, bad]).astype(np.float32)
    return allp[floaters_order(seed)], r


def floaters_order(seed=3):
    return np.random.default_rng(seed + 100).permutation(3000 + N_ISOLATED + N_DUPLICATES + 3)


def floaters_rows(seed=3):
    """dict of bool masks over the rows of floaters(): isolated, duplicate (the added copies), bad (not finite)."""
    kind = np.concatenate([np.zeros(3000, int), np.ones(N_ISOLATED, int), 2 * np.ones(N_DUPLICATES, int), 3 * np.ones(3, int)])
    kind = kind[floaters_order(seed)]
    return dict(isolated=kind == 1, duplicate=kind == 2, bad=kind == 3)


def ragged(M):
    def make():
        return np.random.default_rng(1000 + M).random((M, 3)).astype(np.float32) * 2.0 - 1.0, 0.2
    return make


def line():
    """500 points 0.005 apart on a line that is parallel to no axis: two eigenvalues of every covariance are (nearly) 0."""
    t = 0.005 * np.arange(500)[:, None]
    return (np.array([1.0, 1.0, 1.0]) + t * np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)).astype(np.float32), 0.05


RAGGED = (1, 2, 255, 256, 257, 1025)
SCENES = {"plane": plane, "sphere": sphere, "lattice": lattice, "lattice_diagonal": lattice_diagonal, "ball": ball,
          "floaters": floaters, "line": line, **{f"ragged{M}": ragged(M) for M in RAGGED}}
