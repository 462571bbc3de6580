"""A numpy restatement of the k-nearest-neighbour rule of include/m3slam.h (section "point cloud", the m3_knn_* text),
written from that text: brute force over all pairs in float64, no cells - the only use of the cell edge is the range
test of a point or a query, which the rule defines by it.  index, dist2, found, the statistical filter's q, its sums,
its threshold and the rows it keeps, and the moments over the k nearest, as the device must give them byte for byte.
Scenes of a few thousand points: the distance matrix is built in chunks of queries."""
import math

import numpy as np

ROW_BITS = 30
ROW_MASK = np.uint64((1 << ROW_BITS) - 1)
MAX_K = 64


def radius32(radius):
    return float(np.float32(radius))


def in_range(p, radius):
    """(finite, far): rows whose coordinates are finite; finite rows with |floor((double)p / h)| >= 2^20 on some axis."""
    p = np.asarray(p, np.float32)
    h = radius32(radius) * (1.0 + 2.0 ** -10)
    finite = np.isfinite(p).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor(p.astype(np.float64) / h)
        far = finite & ~(np.abs(c) < 2.0 ** 20).all(axis=1)
    return finite, far


def pack_key(d2, row):
    """(bits(d2) & ~(2^30 - 1)) | row, uint64; d2 non-negative float64."""
    bits = np.ascontiguousarray(d2, dtype=np.float64).view(np.uint64)
    return (bits & ~ROW_MASK) | np.asarray(row, dtype=np.uint64)


def squared_distances(P, q):
    """d2 [len(q), len(P)] = (dx dx + dy dy) + dz dz with d = P - q, every operation a float64 one."""
    d = P[None, :, :] - q[:, None, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def ranked(points, radius, queries=None, chunk=256):
    """The up to 65 smallest keys of every query, ascending, padded with ~0: dict(keys uint64 [Q,65], d2 float64
    [Q,65] (inf where padded), ncand int64 [Q], out_of_range: the finite queries (cross mode) or points (self mode)
    without a cell).  knn() slices it: the k nearest are a prefix of the k + 1 nearest."""
    points = np.ascontiguousarray(points, dtype=np.float32)
    self_mode = queries is None
    Q32 = points if self_mode else np.ascontiguousarray(queries, dtype=np.float32)
    r = radius32(radius)
    fin, far = in_range(points, radius)
    rows = np.flatnonzero(fin & ~far)                                           # the points that can be candidates
    P = points[rows].astype(np.float64)
    qfin, qfar = in_range(Q32, radius)
    nq, width = len(Q32), MAX_K + 1
    keys = np.full((nq, width), ~np.uint64(0), np.uint64)
    d2s = np.full((nq, width), np.inf)
    ncand = np.zeros(nq, np.int64)
    for a in range(0, nq, chunk):
        idx = np.arange(a, min(a + chunk, nq))
        live = idx[qfin[idx] & ~qfar[idx]]
        if not len(live) or not len(rows):
            continue
        d2 = squared_distances(P, Q32[live].astype(np.float64))
        cand = d2 <= r * r
        if self_mode:
            cand &= rows[None, :] != live[:, None]
        key = np.where(cand, pack_key(d2, np.broadcast_to(rows[None, :], d2.shape)), ~np.uint64(0))
        order = np.argsort(key, axis=1, kind="stable")[:, :width]
        n = min(width, key.shape[1])
        keys[live, :n] = np.take_along_axis(key, order, axis=1)
        d2s[live, :n] = np.where(np.take_along_axis(cand, order, axis=1), np.take_along_axis(d2, order, axis=1), np.inf)
        ncand[live] = cand.sum(axis=1)
    return dict(keys=keys, d2=d2s, ncand=ncand, out_of_range=int((far if self_mode else qfar).sum()),
                points_out_of_range=int(far.sum()))


def knn(rk, k):
    """dict(index int32 [Q,k], dist2 float32 [Q,k], found int32 [Q]) of a ranked() result."""
    assert 1 <= k <= MAX_K
    found = np.minimum(rk["ncand"], k).astype(np.int32)
    has = np.arange(k)[None, :] < found[:, None]
    index = np.where(has, (rk["keys"][:, :k] & ROW_MASK).astype(np.int64), -1).astype(np.int32)
    dist2 = np.where(has, rk["d2"][:, :k], np.inf).astype(np.float32)
    return dict(index=index, dist2=dist2, found=found)


def distance_bits_tie(rk, k):
    """True for the queries where two of the first k + 1 keys agree in everything but the row."""
    top = rk["keys"][:, :k + 1]
    real = top != ~np.uint64(0)
    same = ((top[:, 1:] & ~ROW_MASK) == (top[:, :-1] & ~ROW_MASK)) & real[:, 1:] & real[:, :-1]
    return same.any(axis=1)


def isqrt_sum(points, radius, nn, k):
    """q int32 [M]: for a complete row the sum of floor(sqrt(rint(d2 * 2^32 / r^2))) over its k neighbours, else -1."""
    points = np.asarray(points, np.float32)
    r = radius32(radius)
    factor = 2.0 ** 32 / (r * r)
    q = np.full(len(points), -1, np.int32)
    P = points.astype(np.float64)
    for i in np.flatnonzero(nn["found"] == k):
        d = P[nn["index"][i].astype(np.int64)] - P[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        q[i] = sum(math.isqrt(int(v)) for v in np.rint(d2 * factor))
    return q


def statistics(q, std_ratio):
    """dict(n, S1, S2, T, kept): exact integer sums over the complete rows, T in float64 from them, the rows kept."""
    vals = [int(v) for v in q if v >= 0]
    n, s1, s2 = len(vals), sum(vals), sum(v * v for v in vals)
    if n == 0:
        return dict(n=0, S1=0, S2=0, T=-1.0, kept=np.zeros(0, np.int64))
    mu = s1 / n
    var = (n * s2 - s1 * s1) / (n * (n - 1)) if n >= 2 else 0.0
    T = mu + float(std_ratio) * math.sqrt(var)
    kept = np.flatnonzero((q >= 0) & (q.astype(np.float64) <= T)).astype(np.int64)
    return dict(n=n, S1=s1, S2=s2, T=T, kept=kept)


def moments(points, radius, nn):
    """(count int32 [M], moments int64 [M,9]) over i and its found nearest: q = rint(d * 2^20 / r) as integers."""
    points = np.asarray(points, np.float32)
    r = radius32(radius)
    scale = 2.0 ** 20 / r
    fin, far = in_range(points, radius)
    P = points.astype(np.float64)
    count = np.zeros(len(points), np.int32)
    mom = np.zeros((len(points), 9), np.int64)
    for i in np.flatnonzero(fin & ~far):
        j = nn["index"][i, :nn["found"][i]].astype(np.int64)
        o = np.rint((P[j] - P[i]) * scale).astype(np.int64)
        count[i] = len(j) + 1
        mom[i, :3] = o.sum(axis=0)
        mom[i, 3:] = [(o[:, a] * o[:, b]).sum() for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return count, mom


# ---- the small scenes added to those of cloud_twin: (points float32 [M,3], radius) -----------------------------------
def single():
    return np.array([[0.25, -1.0, 3.0]], np.float32), 0.5


def pair():
    return np.array([[0.25, -1.0, 3.0], [0.5, -1.0, 3.0]], np.float32), 0.5


def five():
    """k > M - 1 for every k above 4."""
    return np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.25, 0], [0, 0, -1], [2, 0, 0]], np.float32), 1.0


def dropped_bits():
    """Seen from row 2 at the origin, row 0 is farther than row 1 by one float32 ulp of the coordinate: d2 = 0.5625 +
    1.5 * 2^-24 + 2^-48 against 0.5625.  The kept bits of a d2 in [0.5, 1) step by 2^-23 and 0.5625 lies on a step, so the
    two differ only in the 30 dropped bits - and the key puts the lower row 0, the farther point, first."""
    b = np.float32(0.75)
    a = np.nextafter(b, np.float32(1))
    return np.array([[a, 0, 0], [b, 0, 0], [0, 0, 0]], np.float32), 1.0


def duplicates():
    """300 exact copies of one point and 40 others around it: more ties than any k."""
    g = np.random.default_rng(77)
    one = np.array([[0.3, 0.7, -0.2]], np.float32)
    others = (one + 0.05 * g.normal(size=(40, 3))).astype(np.float32)
    p = np.concatenate([np.repeat(one, 300, axis=0), others])
    return p[g.permutation(len(p))], 0.2


SMALL = {"single": single, "pair": pair, "five": five, "dropped_bits": dropped_bits, "duplicates": duplicates}
