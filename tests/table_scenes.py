"""Inputs that make the shared key table (csrc/table_dev.h) wrap: several distinct keys whose home slot is the last one,
S - 1, of a table of S = 1024 slots, so that a probe chain runs past the end and goes on at slot 0.  mix64 and the two key
packings are restated in numpy; the scenes are small enough that every table they fill has 1024 slots."""
import numpy as np

import components_twin as CC

S = 1024
CELL_BIAS = 1 << 20
U64 = np.uint64


def mix64(x):
    """splitmix64's finaliser on uint64 values, wrapping as the device does."""
    x = np.asarray(x, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> U64(30)
        x *= U64(0xbf58476d1ce4e5b9)
        x ^= x >> U64(27)
        x *= U64(0x94d049bb133111eb)
        return x ^ (x >> U64(31))


def home(keys, slots=S):
    return (mix64(keys) & U64(slots - 1)).astype(np.int64)


def edge_keys(a, b):
    """lo << 31 | hi of the pairs (a, b), in either order."""
    lo, hi = np.minimum(a, b).astype(np.uint64), np.maximum(a, b).astype(np.uint64)
    return (lo << U64(31)) | hi


def cell_keys(cells):
    """The biased 21-bit-per-axis key of integer cells [n,3]."""
    b = (np.asarray(cells).astype(np.int64) + CELL_BIAS).astype(np.uint64)
    return (b[:, 0] << U64(42)) | (b[:, 1] << U64(21)) | b[:, 2]


def last_slot_keys(keys, slots=S):
    """The distinct keys whose home is the last slot."""
    keys = np.unique(np.asarray(keys, dtype=np.uint64))
    return keys[home(keys, slots) == slots - 1]


def hot_edges(V=600):
    """The pairs lo < hi < V whose key homes at slot S - 1, int64 [n,2] in lexicographic order."""
    lo, hi = np.triu_indices(V, 1)
    at = home(edge_keys(lo, hi)) == S - 1
    return np.stack([lo[at], hi[at]], axis=1).astype(np.int64)


def hot_cells(lo=-8, hi=8):
    """The cells of the cube [lo, hi)^3 whose key homes at slot S - 1, int64 [n,3]."""
    r = np.arange(lo, hi)
    c = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    return c[home(cell_keys(c)) == S - 1]


def smooth_mesh(V=600, hot=6, strip=160, seed=3):
    """(vertices, colors, faces): `hot` faces whose first edge homes at the last slot, then the strip of
    components_twin over the first strip + 2 rows.  F <= 170: the edge table has 1024 slots."""
    e = hot_edges(V)
    e = e[np.linspace(0, len(e) - 1, hot).astype(np.int64)]                     # spread over the rows, distinct
    third = (e[:, 1] + 7) % V
    third = np.where((third == e[:, 0]) | (third == e[:, 1]), (third + 1) % V, third)
    faces = np.concatenate([np.stack([e[:, 0], e[:, 1], third], axis=1), CC.strip_faces(strip)]).astype(np.int32)
    rng = np.random.default_rng(seed)
    return rng.normal(size=(V, 3)).astype(np.float32), np.zeros((V, 3), np.uint8), faces


def _in_cells(edge, seed):
    """Positions in the hot cells and the 26 cells around each: two per cell, four in a hot one.  float64 [n,3], in units
    of the cell edge."""
    rng = np.random.default_rng(seed)
    off = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    cells = np.concatenate([np.repeat(h[None, :] + off, 2, axis=0) for h in hot_cells()] + [np.repeat(hot_cells(), 2, axis=0)])
    return (cells + rng.uniform(0.25, 0.75, size=cells.shape)) * edge


CLOUD_RADIUS = float(np.float32(1.0 / (1.0 + 2.0 ** -10)))                    # the cell edge is 1 to a few parts in 10^8


def cloud_points(seed=4):
    """float32 [M,3], M <= 512, a few points in every hot cell and its neighbours at cell edge 1."""
    return _in_cells(CLOUD_RADIUS * (1.0 + 2.0 ** -10), seed).astype(np.float32)


def cloud_queries(seed=5):
    return _in_cells(CLOUD_RADIUS * (1.0 + 2.0 ** -10), seed)[::2].astype(np.float32)


def simplify_mesh(seed=6, F=300):
    """(vertices, colors, faces) with the vertices in the same cells at voxel_size 1 and random faces over them."""
    v = _in_cells(1.0, seed).astype(np.float32)
    rng = np.random.default_rng(seed + 1)
    return v, rng.integers(0, 256, size=v.shape).astype(np.uint8), rng.integers(0, len(v), size=(F, 3)).astype(np.int32)


def voxel_cloud(seed=7):
    """(points, colors, conf) for the exporter's voxel stage at voxel_size 1: the same cells, confidences with ties."""
    p = _in_cells(1.0, seed).astype(np.float32)
    rng = np.random.default_rng(seed + 1)
    return p, rng.integers(0, 256, size=p.shape).astype(np.uint8), (rng.integers(4, 12, size=len(p)) / 4).astype(np.float32)
