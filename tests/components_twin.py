"""numpy twin of the mesh-components rule of include/m3slam.h (csrc/mesh_components.hip, mast3r_slam/components.py), and
the meshes the tests label.

The twin is label propagation in synchronous rounds, written independently of the kernel's compare-and-swap union-find:
every vertex starts with its own row as its label; a round lowers, for every edge of a valid face, the labels of the two
ends' labels to the smaller of them, then lets every label jump to its label's label until that is stable; rounds repeat
until nothing changes.  label[v] <= v holds throughout and labels stay inside the component.  At the fixed point the two
ends of every edge agree and label[label[v]] == label[v], so the label is the smallest row of the component.
Everything else is counting."""
from collections import namedtuple

import numpy as np

Info = namedtuple("Info", ["components", "largest", "winner"])


# ---- the rule --------------------------------------------------------------------------------------------------------
def valid_faces(faces, V):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(axis=1)


def _lower(lab, idx, val):
    """lab[idx] = min(lab[idx], val) with repeated idx (a sort and a segmented minimum: no ufunc.at)."""
    order = np.argsort(idx, kind="stable")
    i, v = idx[order], val[order]
    starts = np.flatnonzero(np.r_[True, i[1:] != i[:-1]])
    rows = i[starts]
    lab[rows] = np.minimum(lab[rows], np.minimum.reduceat(v, starts))


def labels_of(faces, V):
    """label int32 [V]: the smallest row of every vertex's component.  Invalid faces connect nothing."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = f[valid_faces(f, V)]
    e0, e1 = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
    lab = np.arange(V, dtype=np.int64)
    while e0.size:
        new = lab.copy()
        r0, r1 = lab[e0], lab[e1]
        m = np.minimum(r0, r1)
        _lower(new, r0, m)
        _lower(new, r1, m)
        while True:
            jump = new[new]
            if np.array_equal(jump, new):
                break
            new = jump
        if np.array_equal(new, lab):
            break
        lab = new
    return lab.astype(np.int32)


def components(faces, V):
    """(labels int32 [V], faces_of int32 [V] - the count of each vertex's component -, Info, invalid faces)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = valid_faces(f, V)
    lab = labels_of(f, V)
    at_root = np.bincount(lab[f[ok, 0]], minlength=V).astype(np.int64) if V else np.zeros(0, dtype=np.int64)
    largest = int(at_root.max()) if V else 0
    winner = int(np.argmax(at_root)) if largest > 0 else -1                 # argmax: the first, i.e. the smallest label
    info = Info(int((at_root > 0).sum()), largest, winner)
    return lab, at_root[lab].astype(np.int32), info, int((~ok).sum())


def kept_components(at_root, info, min_faces=1, min_fraction=0.0, largest_only=False):
    """bool [V]: is the component whose label is this row kept?  at_root[c]: its faces."""
    keep = at_root >= max(1, int(min_faces))
    fraction = np.float32(min_fraction)
    if fraction != 0:
        keep &= at_root.astype(np.float64) >= np.float64(fraction) * np.float64(info.largest)
    if largest_only:
        keep &= np.arange(at_root.shape[0]) == info.winner
    return keep


def filter_mesh(vertices, colors, faces, min_faces=1, min_fraction=0.0, largest_only=False):
    """(vertices, colors, faces int32, vertex_rows int64, face_rows int64) of the kept components; ValueError for a face
    with a row outside [0, V), as the host raises it."""
    V = vertices.shape[0]
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    lab, of, info, invalid = components(f, V)
    if invalid:
        raise ValueError(f"{invalid} invalid faces")
    at_root = np.where(lab == np.arange(V), of, 0).astype(np.int64)
    keep_c = kept_components(at_root, info, min_faces, min_fraction, largest_only)
    keep_v = keep_c[lab] if V else np.zeros(0, dtype=bool)
    keep_f = keep_c[lab[f[:, 0]]] if f.shape[0] else np.zeros(0, dtype=bool)
    remap = np.cumsum(keep_v) - 1
    rows_v, rows_f = np.flatnonzero(keep_v).astype(np.int64), np.flatnonzero(keep_f).astype(np.int64)
    return vertices[rows_v], colors[rows_v], remap[f[rows_f]].astype(np.int32).reshape(-1, 3), rows_v, rows_f


def bfs_labels(faces, V):
    """Pure-Python breadth-first search: the check of the twin on small meshes."""
    nbr = [[] for _ in range(V)]
    for a, b, c in np.asarray(faces).reshape(-1, 3).tolist():
        if 0 <= a < V and 0 <= b < V and 0 <= c < V:
            for p, q in ((a, b), (b, c), (c, a)):
                nbr[p].append(q)
                nbr[q].append(p)
    lab = [-1] * V
    for s in range(V):                                                       # ascending: the start is the smallest row
        if lab[s] >= 0:
            continue
        lab[s], todo = s, [s]
        while todo:
            nxt = []
            for p in todo:
                for q in nbr[p]:
                    if lab[q] < 0:
                        lab[q] = s
                        nxt.append(q)
            todo = nxt
    return np.asarray(lab, dtype=np.int32)


# ---- meshes ----------------------------------------------------------------------------------------------------------
def arrays(V, seed):
    """vertices float32 [V,3] and colours uint8 [V,3]: random bytes that a copy must preserve (a NaN and a -0 among them)."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((V, 3)).astype(np.float32)
    if V > 2:
        v[1, 0], v[2, 1] = np.nan, -0.0
    return v, rng.integers(0, 256, (V, 3), dtype=np.uint8)


def strip_faces(n, first=0):
    """A strip of n triangles over the n + 2 rows from `first`: triangle i = (i, i + 1, i + 2)."""
    i = np.arange(n, dtype=np.int64)[:, None] + first
    return (i + np.arange(3)[None]).astype(np.int32)


def strip(n, order, seed=0):
    """One strip of n triangles whose rows are a fixed random permutation ("shuffled"), descend along the strip
    ("descending") or ascend ("ascending"); faces in a shuffled order."""
    rng = np.random.default_rng(seed)
    V = n + 2
    perm = {"shuffled": rng.permutation(V), "descending": np.arange(V)[::-1], "ascending": np.arange(V)}[order]
    faces = perm[strip_faces(n)].astype(np.int32)
    if order == "shuffled":
        faces = faces[rng.permutation(n)]
    return arrays(V, seed + 1) + (np.ascontiguousarray(faces),)


ISLAND_SIZES = (2, 3, 5, 8, 12, 13, 20, 39, 40, 40, 40)                   # three islands share the largest count


def islands(n_single=3000, sizes=ISLAND_SIZES, seed=5):
    """n_single disjoint triangles and one strip per entry of `sizes`, rows and face order shuffled."""
    rng = np.random.default_rng(seed)
    parts, first = [], 0
    for n in (1,) * n_single + tuple(sizes):
        parts.append(strip_faces(n, first))
        first += n + 2
    faces = np.concatenate(parts)
    perm = rng.permutation(first)
    faces = perm[faces][rng.permutation(faces.shape[0])].astype(np.int32)
    return arrays(first, seed + 1) + (np.ascontiguousarray(faces),)


def fans(duplicated, n=7, seed=9):
    """Two fans of n triangles around rows 0 and n + 2 that share exactly one rim vertex, row n + 1.  duplicated: the
    second fan names a copy of that vertex in a row of its own, at identical coordinates."""
    rim_a = np.arange(1, n + 2)                                              # rows 1 ... n + 1
    a = np.stack([np.zeros(n, dtype=np.int64), rim_a[:-1], rim_a[1:]], axis=1)
    c = n + 2
    rim_b = np.concatenate([[n + 1], np.arange(c + 1, c + 1 + n)])           # starts at the shared row
    b = np.stack([np.full(n, c), rim_b[:-1], rim_b[1:]], axis=1)
    V = c + 1 + n
    v, col = arrays(V + (1 if duplicated else 0), seed)
    if duplicated:
        b[b == n + 1] = V                                                    # the twin row
        v[V], col[V] = v[n + 1], col[n + 1]
    return v, col, np.concatenate([a, b]).astype(np.int32)


def with_unreferenced(mesh, where):
    """The mesh with a vertex no face names inserted before each input row in `where` (V: at the end)."""
    v, c, f = mesh
    where = np.sort(np.asarray(where, dtype=np.int64))
    v2, c2 = np.insert(v, where, np.float32(7.5), axis=0), np.insert(c, where, np.uint8(9), axis=0)
    shift = np.searchsorted(where, np.arange(v.shape[0]), side="right")      # inserted rows at or before each input row
    return v2, c2, (f + shift[f]).astype(np.int32)


def scattered_triangles(V, n, seed, tail=2):
    """n disjoint triangles on random rows of V, and a strip of `tail` triangles on the last tail + 2 rows; every other
    row is named by no face."""
    rng = np.random.default_rng(seed)
    rows = rng.permutation(V - (tail + 2))[:3 * n].reshape(n, 3)
    faces = np.concatenate([rows, strip_faces(tail, V - (tail + 2))])
    faces = faces[rng.permutation(faces.shape[0])].astype(np.int32)
    return arrays(V, seed + 1) + (np.ascontiguousarray(faces),)
