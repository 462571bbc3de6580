"""The vertex-clustering rule of include/m3slam.h (section "mesh simplify") restated in numpy, written from that text and
not from the kernel, and the scenes the simplify tests share.  Every float64 operation is one numpy operation, so it is
rounded on its own, as the header asks; the sums are int64.  Needs no GPU."""
import numpy as np

CELL_LIM = float(2 ** 20)
Q = float(2 ** 24)


def voxel_of(voxel_size):
    """voxel_size rounded to fp32 once, then float64."""
    return np.float64(np.float32(voxel_size))


def cells_of(vertices, voxel_size):
    """(cell int64 [V,3], q int64 [V,3], in_range bool [V]); cell and q are 0 where the vertex is out of range."""
    voxel = voxel_of(voxel_size)
    with np.errstate(invalid="ignore", over="ignore"):
        t = vertices.astype(np.float64) / voxel
        c = np.floor(t)
        ok = (np.isfinite(vertices) & (np.abs(c) < CELL_LIM)).all(axis=1)       # NaN compares false
        t, c = np.where(ok[:, None], t, 0.0), np.where(ok[:, None], c, 0.0)
        q = np.rint((t - c) * Q).astype(np.int64)                               # round to nearest even
    return c.astype(np.int64), q, ok


def rotate_min_first(tri):
    """Each row rotated so that its smallest entry comes first (the rows have three different entries)."""
    tri = np.asarray(tri)
    if tri.shape[0] == 0:
        return tri.reshape(0, 3).copy()
    k = np.argmin(tri, axis=1)
    cols = (k[:, None] + np.arange(3)[None, :]) % 3
    return np.take_along_axis(tri, cols, axis=1)


def simplify(vertices, colors, faces, voxel_size):
    """(vertices float32 [V2,3], colors uint8 [V2,3], faces int32 [F2,3], cluster_of int64 [V], face_rows int64 [F2],
    info) with info = dict(out_of_range, invalid, sizes int64 [V2], collapsed, out_faces, repeats).  ValueError when a face
    names a row outside [0, V), as the Python layer raises."""
    vertices, colors, faces = np.asarray(vertices), np.asarray(colors), np.asarray(faces)
    V, F = vertices.shape[0], faces.shape[0]
    voxel = voxel_of(voxel_size)
    cell, q, ok = cells_of(vertices, voxel_size)
    rows = np.flatnonzero(ok)
    # clusters: the same cell triple; leader = the smallest row; output in ascending leader
    uniq, first, inv = np.unique(cell[rows], axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    leader = rows[first]                                                        # np.unique: index of the first occurrence
    order = np.argsort(leader, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(order.shape[0])
    cluster_of = np.full((V,), -1, dtype=np.int64)
    cluster_of[rows] = rank[inv]
    V2 = order.shape[0]
    leader, ccell = leader[order], uniq[order]
    n = np.bincount(cluster_of[rows], minlength=V2).astype(np.int64)
    S = np.zeros((V2, 3), dtype=np.int64)
    C = np.zeros((V2, 3), dtype=np.int64)
    np.add.at(S, cluster_of[rows], q[rows])
    np.add.at(C, cluster_of[rows], colors[rows].astype(np.int64))
    out_v = vertices[leader].copy()                                             # n = 1: the vertex's own bits and colour
    out_c = colors[leader].copy()
    many = n > 1
    den = n[many].astype(np.float64) * Q
    mean = S[many].astype(np.float64) / den[:, None]
    out_v[many] = ((ccell[many].astype(np.float64) + mean) * voxel).astype(np.float32)
    out_c[many] = ((2 * C[many] + n[many, None]) // (2 * n[many, None])).astype(np.uint8)
    # faces
    valid = ((faces >= 0) & (faces < V)).all(axis=1) if F else np.zeros((0,), dtype=bool)
    invalid = int(F - valid.sum())
    info = dict(out_of_range=int(V - rows.shape[0]), invalid=invalid, sizes=n)
    if invalid:
        raise ValueError(f"{invalid} faces name a vertex row outside [0, {V})")
    tri = cluster_of[faces.astype(np.int64)].reshape(F, 3)
    in_range = (tri >= 0).all(axis=1)
    distinct = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    cand = np.flatnonzero(in_range & distinct)
    keys = rotate_min_first(tri[cand])
    _, first_f = np.unique(keys, axis=0, return_index=True)                     # the smallest input row of every key
    keep = np.sort(first_f)
    info.update(collapsed=int((in_range & ~distinct).sum()), out_faces=int((~in_range).sum()),
                repeats=int(cand.shape[0] - keep.shape[0]))
    return (out_v.astype(np.float32), out_c.astype(np.uint8), keys[keep].astype(np.int32).reshape(-1, 3), cluster_of,
            cand[keep].astype(np.int64), info)


# ---- scenes ----------------------------------------------------------------------------------------------------------
SPACING = 0.01


def grid_mesh(ny=29, nx=33, seed=5, jitter=0.15, shuffle=True, spacing=SPACING):
    """A jittered ny x nx grid around the plane z = 0, centred on the origin so that all three coordinates lie on both
    sides of zero, two triangles per quad, the vertex rows shuffled: (vertices float32, colors uint8, faces int32)."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(ny) - (ny - 1) / 2.0, np.arange(nx) - (nx - 1) / 2.0, indexing="ij")
    p = np.stack([x, y, np.zeros_like(x)], axis=-1).reshape(-1, 3)
    p = (p + rng.uniform(-jitter, jitter, p.shape)) * spacing
    idx = np.arange(ny * nx).reshape(ny, nx)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    faces = np.concatenate([np.stack([a, b, c], axis=1), np.stack([b, d, c], axis=1)])
    colors = rng.integers(0, 256, (ny * nx, 3)).astype(np.uint8)
    perm = rng.permutation(ny * nx) if shuffle else np.arange(ny * nx)
    where = np.empty_like(perm)
    where[perm] = np.arange(ny * nx)                                            # old row -> new row
    return p[perm].astype(np.float32), colors[perm], where[faces].astype(np.int32)


def boundary_mesh(n=9, voxel=0.25):
    """Vertices exactly on cell boundaries, k * voxel and -k * voxel on both axes, with one more vertex inside every
    other cell so that clusters of two exist; a fan of faces over consecutive rows."""
    k = np.arange(-n, n + 1)
    y, x = np.meshgrid(k, k, indexing="ij")
    on = np.stack([x * voxel, y * voxel, np.zeros_like(x, dtype=np.float64)], axis=-1).reshape(-1, 3)
    inside = on[::2] + np.array([0.4 * voxel, 0.7 * voxel, 0.2 * voxel])
    v = np.concatenate([on, inside]).astype(np.float32)
    rng = np.random.default_rng(11)
    c = rng.integers(0, 256, (v.shape[0], 3)).astype(np.uint8)
    r = np.arange(v.shape[0] - 2)
    f = np.stack([r, r + 1, r + 2], axis=1).astype(np.int32)
    return v, c, f


def with_out_of_range(mesh):
    """mesh with three more vertices - a NaN, an infinity and 1e30 - each named by one more face."""
    v, c, f = mesh
    V = v.shape[0]
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, 1e30]], dtype=np.float32)
    v2 = np.concatenate([v[:5], bad[:1], v[5:], bad[1:]])                       # one in the middle, two at the end
    c2 = np.concatenate([c[:5], c[:1], c[5:], c[:2]])
    shift = lambda a: np.where(a >= 5, a + 1, a)
    f2 = np.concatenate([shift(f), np.array([[5, 0, 1], [2, V + 1, 3], [V + 2, 6, 7]], dtype=np.int32)]).astype(np.int32)
    return v2, c2, f2


def winding_pair(opposite):
    """Six vertices, two per cell of three cells (voxel 1.0), and two faces over the three clusters: the second written
    from another corner, with the same winding or the opposite one."""
    v = np.array([[0.2, 0.2, 0.1], [1.3, 0.1, 0.2], [0.4, 1.6, 0.3], [0.7, 0.6, 0.5], [1.8, 0.9, 0.6], [0.1, 1.2, 0.9]], dtype=np.float32)
    c = (np.arange(18).reshape(6, 3) * 13 % 256).astype(np.uint8)
    second = [5, 4, 3] if opposite else [4, 5, 3]                               # clusters (2, 1, 0) or (1, 2, 0)
    return v, c, np.array([[0, 1, 2], second], dtype=np.int32)
