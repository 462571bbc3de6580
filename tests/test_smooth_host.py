"""CPU: the mesh-smooth rule (tests/smooth_twin.py) against things that do not come from the twin - a scipy.sparse
adjacency matrix, Euler's formula on a closed sphere, the rim of an open grid, an integer lattice on which every sum of
the rule is exact, and what the filter is for (ripples go, the sphere keeps its radius under Taubin and shrinks under
Laplacian); the host checks of mast3r_slam/smooth.py that need no device; and the workspace size, launch count and
argument validation of the C entry points, which happen before any HIP call."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import scipy.sparse
import torch

import smooth_twin as ST
from mast3r_slam import _ffi, mast3r_utils, smooth


@pytest.fixture(scope="module")
def built_lib():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(_ffi.LIB_PATH):
        spec = importlib.util.spec_from_file_location("m3build", os.path.join(root, "mast3r-slam_amd", "build.py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        m.build(verbose=False)
    return ctypes.CDLL(_ffi.LIB_PATH)


# ---- the twin --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", sorted(ST.SCENES))
def test_adjacency_against_a_sparse_matrix(scene):
    v, _, f = ST.SCENES[scene]()
    V = len(v)
    good = f[((f >= 0) & (f < V)).all(axis=1)].astype(np.int64)
    src = np.concatenate([good[:, 0], good[:, 1], good[:, 2], good[:, 1], good[:, 2], good[:, 0]])
    dst = np.concatenate([good[:, 1], good[:, 2], good[:, 0], good[:, 0], good[:, 1], good[:, 2]])
    keep = src != dst
    A = scipy.sparse.coo_matrix((np.ones(int(keep.sum())), (src[keep], dst[keep])), shape=(V, V)).tocsr()
    A.data[:] = 1.0                                                             # repeated entries were summed: 0 / 1
    A.sort_indices()
    off, nbr = ST.adjacency(f, V)
    top = ST.topology(f, V)
    assert np.array_equal(np.asarray(A.sum(axis=1)).reshape(-1).astype(np.int32), top["degree"])
    assert np.array_equal(A.indptr, off) and np.array_equal(A.indices, nbr)
    assert top["edges"] * 2 == len(nbr) == A.nnz
    for r in range(V):                                                          # ascending and unique
        row = nbr[off[r]:off[r + 1]]
        assert (np.diff(row) > 0).all() and r not in row


def test_odd_faces_are_counted_as_the_header_says():
    v, _, f = ST.odd_faces()
    n = 12 * 11
    top = ST.topology(f, len(v))
    rows = {tuple(r): int(c) for r, c in zip(top["edge_rows"], top["edge_faces"])}
    assert rows[(n, n + 1)] == 3 and top["nonmanifold_edges"] == 4              # three faces on one edge; the face given
    assert rows[(n + 5, n + 6)] == rows[(n + 6, n + 7)] == rows[(n + 5, n + 7)] == 3     # three times, either winding
    assert rows[(n + 2, n + 3)] == 2                                            # (a, a, b): the corners a-b and b-a
    assert top["degree"][n + 8] == 0 and top["degree"][n + 4] == 2              # isolated; (a, a, a) adds nothing
    assert top["invalid_faces"] == 0
    bad = np.concatenate([f, [[0, 1, len(v)], [-1, 0, 1]]]).astype(np.int32)
    t2 = ST.topology(bad, len(v))
    assert t2["invalid_faces"] == 2 and np.array_equal(t2["edge_rows"], top["edge_rows"])


def test_closed_sphere():
    v, _, f = ST.icosphere()
    assert v.shape == (642, 3) and f.shape == (1280, 3)
    top = ST.topology(f, len(v))
    assert top["edges"] == 3 * len(f) // 2 == 1920 and len(v) - top["edges"] + len(f) == 2
    assert top["boundary_edges"] == 0 and top["nonmanifold_edges"] == 0 and not top["boundary"].any()
    assert (top["edge_faces"] == 2).all() and sorted(set(top["degree"])) == [5, 6]


def test_open_grid():
    v, _, f = ST.jittered_grid()
    top = ST.topology(f, len(v))
    assert len(v) == 1200 and np.array_equal(top["boundary"], ST.grid_rim())
    assert top["boundary_edges"] == 2 * (40 - 1) + 2 * (30 - 1) and top["nonmanifold_edges"] == 0


def test_integer_lattice_is_exact():
    v, _, f = ST.integer_lattice()
    rim = ST.grid_rim(9, 9)
    for it in (1, 4, 10):
        assert ST.smooth(v, f, iterations=it, method="taubin", fix_boundary=True).tobytes() == v.tobytes()
    one = ST.smooth(v, f, iterations=1, method="laplacian")
    assert (~rim).sum() == 49 and one[~rim].tobytes() == v[~rim].tobytes() and one[rim].tobytes() != v[rim].tobytes()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_what_the_filter_is_for(seed):
    v, _, f = ST.noisy_icosphere(seed)
    radius = lambda p: np.linalg.norm(p.astype(np.float64), axis=1)
    r0 = radius(v)
    rt = radius(ST.smooth(v, f, iterations=10, method="taubin"))
    rl = radius(ST.smooth(v, f, iterations=10, method="laplacian"))
    print(f"seed {seed}: taubin std ratio {rt.std() / r0.std():.4f}, mean radius {r0.mean():.5f} -> {rt.mean():.5f}; "
          f"laplacian mean radius {rl.mean():.5f}")
    assert rt.std() < 0.5 * r0.std()
    assert abs(rt.mean() - r0.mean()) < 0.01
    assert rl.mean() < 0.96


def test_pass_details():
    v, _, f = ST.odd_faces()
    out = ST.smooth(v, f, iterations=3)
    for r in (ST.ODD_NAN, ST.ODD_INF, len(v) - 1):                              # not finite, and isolated: bit for bit
        assert out[r].tobytes() == v[r].tobytes()
    assert np.isfinite(out[np.isfinite(v).all(axis=1)]).all()                   # a NaN neighbour is skipped, not added
    pin = np.zeros(len(v), bool)
    pin[::3] = True
    out = ST.smooth(v, f, iterations=2, method="laplacian", pinned=pin)
    assert out[pin].tobytes() == v[pin].tobytes()
    assert ST.smooth(v, f, iterations=0).tobytes() == v.tobytes()
    v2, _, f2 = ST.jittered_grid()
    assert ST.smooth(v2, f2, iterations=2).tobytes() == ST.smooth(v2, ST.shuffled(f2, 99), iterations=2).tobytes()
    # float64 sums: on the offset grid a float32 sum of the neighbours gives other bytes
    v3, _, f3 = ST.offset_grid()
    off, nbr = ST.adjacency(f3, len(v3))
    s32 = np.stack([v3[nbr[off[r]:off[r + 1]]].sum(axis=0, dtype=np.float32) / np.float32(off[r + 1] - off[r]) for r in range(len(v3))])
    lap32 = (v3 + np.float32(0.5) * (s32 - v3)).astype(np.float32)
    assert lap32.tobytes() != ST.smooth(v3, f3, iterations=1, method="laplacian").tobytes()


# ---- host checks -----------------------------------------------------------------------------------------------------
def test_cpu_tensors_and_bad_arguments(monkeypatch):
    v, c, f = (torch.from_numpy(a) for a in ST.integer_lattice())
    # arguments that cannot be used are refused before the library is needed
    monkeypatch.setattr(_ffi, "lib", lambda: pytest.fail("the library was loaded"))
    nan, inf = float("nan"), float("inf")
    for kw in (dict(iterations=-1), dict(iterations=1.5), dict(iterations=None), dict(method="cotangent"), dict(method=None),
               dict(lam=0.0), dict(lam=-0.5), dict(lam=1.5), dict(lam=nan), dict(lam=inf), dict(lam=1e-60), dict(mu=nan),
               dict(mu=inf), dict(mu=-inf), dict(mu=1e60), dict(pinned=torch.zeros(len(v), dtype=torch.uint8)),
               dict(pinned=torch.zeros((len(v), 1), dtype=torch.bool)), dict(pinned=np.zeros(len(v), bool))):
        with pytest.raises(ValueError):
            smooth.smooth_mesh(v, c, f, **kw)
        with pytest.raises(ValueError):
            smooth.smooth_mesh((v, c, f), **kw)
    for args in ((v, c[:-1], f), (v, c, f.to(torch.int64)), (v.double(), c, f), (v, c.to(torch.int8), f), (v, c, f.reshape(-1)),
                 ((v, c, f), c, f), ((v, c),), (v.numpy(), c, f), (v, c, None)):
        with pytest.raises(ValueError):
            smooth.smooth_mesh(*args)
    for call in (lambda: smooth.smooth_mesh(v, c, f), lambda: smooth.smooth_mesh((v, c, f), iterations=0, method="laplacian"),
                 lambda: smooth.smooth_mesh(v, c, f, pinned=torch.zeros(len(v), dtype=torch.bool)),
                 lambda: smooth.mesh_topology(f, len(v)), lambda: smooth.mesh_topology(f, len(v), return_edges=True)):
        with pytest.raises(RuntimeError, match="ROCm device"):
            call()
    for args in ((f.to(torch.int64), 81), (f.reshape(-1), 81), (f.numpy(), 81), ((v, c, f), 81), (f, -1), (f, 2 ** 31)):
        with pytest.raises(ValueError):
            smooth.mesh_topology(*args)


def test_re_exports_and_signatures():
    for n in ("smooth_mesh", "mesh_topology", "MeshTopology"):
        assert n in mast3r_utils.__all__ and n in smooth.__all__ and getattr(mast3r_utils, n) is getattr(smooth, n)
    assert "workspace_bytes" in smooth.__all__
    E = inspect.Parameter.empty
    sig = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    assert sig(smooth.smooth_mesh) == [("vertices", E), ("colors", None), ("faces", None), ("iterations", 10), ("method", "taubin"),
                                       ("lam", 0.5), ("mu", -0.53), ("fix_boundary", False), ("pinned", None), ("workspace", None)]
    assert sig(smooth.mesh_topology) == [("faces", E), ("n_vertices", E), ("return_edges", False), ("workspace", None)]
    assert sig(smooth.workspace_bytes) == [("n_vertices", E), ("n_faces", E)]
    assert smooth.MeshTopology._fields == ("edges", "boundary_edges", "nonmanifold_edges", "invalid_faces", "degree", "boundary",
                                           "edge_rows", "edge_faces")


def test_symbols_workspace_launches_and_argument_validation(built_lib):
    names = [n for n in _ffi.declared_symbols() if n.startswith(("m3_mesh_smooth", "m3_mesh_topology"))]
    assert sorted(names) == ["m3_mesh_smooth_launches", "m3_mesh_smooth_passes", "m3_mesh_smooth_ws_bytes",
                             "m3_mesh_topology_build", "m3_mesh_topology_edges", "m3_mesh_topology_read"]
    for n in names:
        assert hasattr(built_lib, n), n
    L = _ffi.lib()
    assert L.m3_mesh_smooth_launches() == 7
    pad = lambda b: (b + 15) // 16 * 16
    tiles = lambda n: (n + 255) // 256

    def slots(n):
        s = 1024
        while s < n:
            s *= 2
        return s

    fmax = (2 ** 31 - 1) // 6
    for V, F in ((0, 0), (1, 1), (5, 0), (0, 5), (257, 1023), (642, 1280), (78302, 152882), (1 << 20, (1 << 21) + 3),
                 (2 ** 31 - 1, fmax)):
        S = slots(6 * F)
        want = 64 + pad(4 * tiles(V + 1)) + pad(4 * (V + 2)) + 12 * S + pad(V) + pad(12 * F) + 2 * pad(24 * F) + 32 * V
        assert L.m3_mesh_smooth_ws_bytes(V, F) == want == smooth.workspace_bytes(V, F), (V, F)
        assert S >= 2 * 3 * F                                                   # at most half full
    for V, F in ((-1, 4), (4, -1), (2 ** 31, 4), (4, fmax + 1)):
        assert L.m3_mesh_smooth_ws_bytes(V, F) == 0, (V, F)
        with pytest.raises(ValueError):
            smooth.workspace_bytes(V, F)
    one, big = 0x1000, 1 << 40                                                  # never dereferenced: every call below is refused
    nan, inf = float("nan"), float("inf")
    for n in names:                                                             # the prototypes of the header on the raw handle
        getattr(built_lib, n).argtypes, getattr(built_lib, n).restype = getattr(L, n).argtypes, getattr(L, n).restype
    short = L.m3_mesh_smooth_ws_bytes(8, 8) - 1
    build = lambda **k: built_lib.m3_mesh_topology_build(*[k.get(n, d) for n, d in (
        ("faces", one), ("V", 8), ("F", 8), ("ws", one), ("ws_bytes", big), ("stream", None))])
    for bad in (dict(faces=None), dict(ws=None), dict(V=-1), dict(F=-1), dict(V=2 ** 31), dict(F=fmax + 1), dict(ws=one + 8),
                dict(ws_bytes=short), dict(faces=one + 2)):
        assert build(**bad) == -1, bad
    read = lambda **k: built_lib.m3_mesh_topology_read(*[k.get(n, d) for n, d in (
        ("ws", one), ("V", 8), ("F", 8), ("degree", one), ("boundary", one), ("stream", None))])
    for bad in (dict(ws=None), dict(ws=one + 4), dict(V=-1), dict(F=fmax + 1), dict(degree=None), dict(boundary=None),
                dict(degree=one + 2)):
        assert read(**bad) == -1, bad
    edges = lambda **k: built_lib.m3_mesh_topology_edges(*[k.get(n, d) for n, d in (
        ("ws", one), ("V", 8), ("F", 8), ("E", 12), ("rows", one), ("counts", one), ("stream", None))])
    for bad in (dict(ws=None), dict(ws=one + 4), dict(V=-1), dict(F=-1), dict(E=-1), dict(E=25), dict(rows=None), dict(counts=None),
                dict(rows=one + 2), dict(counts=one + 1)):
        assert edges(**bad) == -1, bad
    passes = lambda **k: built_lib.m3_mesh_smooth_passes(*[k.get(n, d) for n, d in (
        ("vertices", one), ("V", 8), ("F", 8), ("ws", one), ("ws_bytes", big), ("pinned", None), ("fix", 0), ("method", 1),
        ("iterations", 3), ("lam", 0.5), ("mu", -0.53), ("out", 2 * one), ("stream", None))])
    for bad in (dict(vertices=None), dict(out=None), dict(out=one), dict(ws=None), dict(ws=one + 8), dict(ws_bytes=short), dict(V=-1),
                dict(F=fmax + 1), dict(fix=2), dict(method=2), dict(method=-1), dict(iterations=-1), dict(lam=0.0), dict(lam=1.5),
                dict(lam=nan), dict(mu=nan), dict(mu=inf), dict(mu=-inf), dict(vertices=one + 2), dict(out=2 * one + 1)):
        assert passes(**bad) == -1, bad
