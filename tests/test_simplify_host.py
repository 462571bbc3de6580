"""CPU: the vertex-clustering rule (tests/simplify_twin.py) against properties that do not come from the twin - cells
counted with a Python dict, plain float64 means, the face rules checked face by face - on a jittered grid mesh that is
asserted to reach every branch; the host checks of mast3r_slam/simplify.py that need no device; and the workspace size,
launch count and argument validation of the C entry points, which happen before any HIP call."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

import simplify_twin as ST
from mast3r_slam import _ffi, mast3r_utils, simplify

VOXEL = 2.5 * ST.SPACING


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


@pytest.fixture(scope="module")
def grid():
    mesh = ST.grid_mesh()                                                       # 29 x 33, spacing 0.01, jitter 0.15, rows shuffled
    return mesh, ST.simplify(*mesh, VOXEL)


def cell_groups(v, voxel):
    """{cell triple: [rows]} with plain Python floats: math.floor of the float64 quotient."""
    groups = {}
    for i, p in enumerate(v.tolist()):
        groups.setdefault(tuple(math.floor(x / voxel) for x in p), []).append(i)
    return groups


def rotations(t):
    a, b, c = t
    return {(a, b, c), (b, c, a), (c, a, b)}


# ---- the twin --------------------------------------------------------------------------------------------------------
def test_scene_reaches_every_branch(grid):
    (v, c, f), (v2, c2, f2, cluster_of, face_rows, info) = grid
    voxel = float(np.float32(VOXEL))
    assert v.shape == (957, 3) and f.shape == (1792, 3) and (v.min(axis=0) < 0).all() and (v.max(axis=0) > 0).all()
    groups = cell_groups(v, voxel)
    sizes = sorted(len(g) for g in groups.values())
    # counted here without the twin: the cells, the faces whose three rows lie in three cells, and their distinct keys
    cell_of_row = {i: k for k, g in groups.items() for i in g}
    open_faces = [tuple(cell_of_row[i] for i in t) for t in f.tolist()]
    open_faces = [t for t in open_faces if len(set(t)) == 3]
    distinct = {min(rotations(t)) for t in open_faces}
    print(f"{v.shape[0]} -> {len(groups)} vertices ({sizes.count(1)} singletons, largest cluster {sizes[-1]}); "
          f"{f.shape[0]} -> {len(distinct)} faces ({len(open_faces)} survive the collapse test)")
    assert (len(groups), sizes.count(1), sizes[-1]) == (318, 37, 7)
    assert (len(open_faces), len(distinct)) == (749, 747)
    assert v2.shape[0] == 318 and f2.shape[0] == 747 and info["out_of_range"] == 0
    assert sizes.count(1) >= 1 and sizes[-1] >= 4                               # a singleton, a cluster of >= 4
    assert info["collapsed"] == 1792 - 749 >= 1 and info["repeats"] == 2 >= 1   # a collapsed face, a repeated face
    assert sorted(info["sizes"].tolist()) == sizes


def test_vertices_one_per_cell_in_its_box_at_the_mean(grid):
    (v, c, f), (v2, c2, f2, cluster_of, face_rows, info) = grid
    voxel = float(np.float32(VOXEL))
    groups = cell_groups(v, voxel)
    out_cells = [tuple(math.floor(x / voxel) for x in p) for p in v2.tolist()]
    assert len(set(out_cells)) == len(out_cells) == len(groups)                 # no two output vertices share a cell
    leaders = []
    for o, cell in enumerate(out_cells):
        rows = groups[cell]                                                     # KeyError: an output vertex outside every input cell
        leaders.append(min(rows))
        assert (cluster_of[rows] == o).all()
        lo, hi = np.array(cell) * voxel, (np.array(cell) + 1) * voxel
        assert (v2[o] >= np.float32(lo)).all() and (v2[o] <= np.float32(hi)).all()     # in its cell's box, to fp32
        if len(rows) == 1:
            assert v2[o].tobytes() == v[rows[0]].tobytes() and c2[o].tobytes() == c[rows[0]].tobytes()
            continue
        # voxel * 2^-25 from quantising each offset to 2^-24 of the cell, half an fp32 ulp from the final rounding
        mean = v[rows].astype(np.float64).mean(axis=0)
        bound = voxel * 2.0 ** -25 + 0.5 * np.spacing(np.abs(mean).astype(np.float32)).astype(np.float64)
        assert (np.abs(v2[o].astype(np.float64) - mean) <= bound).all(), (o, v2[o], mean)
        want = np.floor(c[rows].astype(np.float64).mean(axis=0) + 0.5)          # the rounded mean: exact at these sizes
        assert np.array_equal(c2[o].astype(np.float64), want)
    assert leaders == sorted(leaders)                                           # clusters in the order of first appearance
    assert cluster_of.min() == 0 and cluster_of.max() == len(groups) - 1


def test_faces_no_collapse_no_repeat_in_order(grid):
    (v, c, f), (v2, c2, f2, cluster_of, face_rows, info) = grid
    assert f2.dtype == np.int32 and face_rows.dtype == np.int64 and cluster_of.dtype == np.int64
    assert (np.diff(face_rows) > 0).all()                                       # increasing
    seen = {}
    for k, t in enumerate(f2.tolist()):
        assert len(set(t)) == 3 and t[0] == min(t)                              # no repeated row; written as the rotated key
        assert tuple(t) not in seen                                             # no two faces with the same key
        seen[tuple(t)] = int(face_rows[k])
        assert tuple(t) in rotations(tuple(cluster_of[f[face_rows[k]]].tolist()))
    # every input face is collapsed, kept, or a later repeat of a kept face with the same rotated key
    kept = set(face_rows.tolist())
    for i, t in enumerate(f.tolist()):
        m = tuple(cluster_of[t].tolist())
        if len(set(m)) < 3:
            assert i not in kept
            continue
        key = min(rotations(m), key=lambda r: r[0])
        assert key in seen and seen[key] <= i and (i in kept) == (seen[key] == i)


def test_small_cases_of_the_rule():
    # opposite winding: both stay; the same winding from another corner: the smaller row stays
    for opposite, want in ((False, [[0, 1, 2]]), (True, [[0, 1, 2], [0, 2, 1]])):
        v2, c2, f2, cluster_of, rows, info = ST.simplify(*ST.winding_pair(opposite), 1.0)
        assert f2.tolist() == want and rows.tolist() == list(range(len(want))) and cluster_of.tolist() == [0, 1, 2, 0, 1, 2]
    v, c, f = ST.winding_pair(False)
    v2, c2, f2, _, _, _ = ST.simplify(v, c, f, 1.0)
    assert c2.tolist() == [[(2 * (int(a) + int(b)) + 2) // 4 for a, b in zip(c[i], c[i + 3])] for i in range(3)]
    # a voxel finer than the mesh: the arrays come back byte for byte, the faces as their rotated keys
    mesh = ST.grid_mesh()
    v2, c2, f2, cluster_of, rows, info = ST.simplify(*mesh, 0.1 * ST.SPACING)
    assert v2.tobytes() == mesh[0].tobytes() and c2.tobytes() == mesh[1].tobytes()
    assert np.array_equal(f2, ST.rotate_min_first(mesh[2])) and np.array_equal(cluster_of, np.arange(957))
    # exactly on cell boundaries, both signs: k * 0.25 lies in cell k
    v = np.array([[k * 0.25, -k * 0.25, 0.0] for k in range(-4, 5)], dtype=np.float32)
    cell, q, ok = ST.cells_of(v, 0.25)
    assert ok.all() and not q.any() and cell[:, 0].tolist() == list(range(-4, 5)) and cell[:, 1].tolist() == list(range(4, -5, -1))
    # out of range: NaN, infinity, a cell at 2^20; the last cell inside is 2^20 - 1
    v = np.array([[np.nan, 0, 0], [0, -np.inf, 0], [0, 0, 1e30], [2.0 ** 20, 0, 0], [-(2.0 ** 20), 0, 0], [2.0 ** 20 - 1, 0, 0],
                  [-(2.0 ** 20) + 1, 0, 0]], dtype=np.float32)
    assert ST.cells_of(v, 1.0)[2].tolist() == [False] * 5 + [True] * 2
    out = ST.simplify(*ST.with_out_of_range(ST.boundary_mesh()), 0.25)
    assert out[5]["out_of_range"] == 3 and out[5]["out_faces"] >= 3 and (out[3] == -1).sum() == 3
    with pytest.raises(ValueError, match="outside"):
        ST.simplify(v, np.zeros((7, 3), np.uint8), np.array([[0, 1, 7]], dtype=np.int32), 1.0)
    empty = ST.simplify(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.int32), 1.0)
    assert [a.shape for a in empty[:5]] == [(0, 3), (0, 3), (0, 3), (0,), (0,)]


# ---- host checks -----------------------------------------------------------------------------------------------------
def test_cpu_tensors_and_bad_arguments(monkeypatch):
    v, c, f = (torch.from_numpy(a) for a in ST.winding_pair(False))
    # a voxel_size that cannot be used is refused before the library is needed
    monkeypatch.setattr(_ffi, "lib", lambda: pytest.fail("the library was loaded"))
    for bad in (None, 0, 0.0, -1.0, float("nan"), float("inf"), -float("inf"), 1e-60, 1e60):     # the last two as fp32: 0, inf
        with pytest.raises(ValueError, match="voxel_size"):
            simplify.simplify_mesh(v, c, f, voxel_size=bad)
        with pytest.raises(ValueError, match="voxel_size"):
            simplify.simplify_counts((v, c, f), voxel_size=bad)
    with pytest.raises(ValueError, match="voxel_size"):
        simplify.simplify_mesh((v, c, f))
    for call in (lambda: simplify.simplify_mesh(v, c, f, voxel_size=1.0), lambda: simplify.simplify_mesh((v, c, f), voxel_size=1.0),
                 lambda: simplify.simplify_counts(v, c, f, voxel_size=1.0)):
        with pytest.raises(RuntimeError, match="ROCm device"):
            call()
    for args in ((v, c[:-1], f), (v, c, f.to(torch.int64)), (v.double(), c, f), (v, c.to(torch.int8), f), (v, c, f.reshape(-1)),
                 ((v, c, f), c, f), ((v, c),), (v.numpy(), c, f), (v, c, None)):
        with pytest.raises(ValueError):
            simplify.simplify_mesh(*args, voxel_size=1.0)


def test_re_exports_and_signatures():
    for n in ("simplify_mesh", "simplify_counts", "SimplifyInfo"):
        assert n in mast3r_utils.__all__ and n in simplify.__all__ and getattr(mast3r_utils, n) is getattr(simplify, n)
    assert "workspace_bytes" in simplify.__all__
    E = inspect.Parameter.empty
    sig = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    assert sig(simplify.simplify_mesh) == [("vertices", E), ("colors", None), ("faces", None), ("voxel_size", None),
                                           ("return_index", False), ("workspace", None)]
    assert sig(simplify.workspace_bytes) == [("n_vertices", E), ("n_faces", E)]
    assert simplify.SimplifyInfo._fields == ("vertices", "faces", "out_of_range")


def test_symbols_workspace_launches_and_argument_validation(built_lib):
    names = [n for n in _ffi.declared_symbols() if n.startswith("m3_mesh_simplify")]
    assert sorted(names) == ["m3_mesh_simplify_count", "m3_mesh_simplify_launches", "m3_mesh_simplify_scatter",
                             "m3_mesh_simplify_ws_bytes"]
    for n in names:
        assert hasattr(built_lib, n), n
    L = _ffi.lib()
    assert L.m3_abi_version() == 4000
    assert L.m3_mesh_simplify_launches() == 8                                   # 6 to count, 2 to scatter
    pad = lambda b: (b + 15) // 16 * 16
    tiles = lambda n: max(1, (n + 255) // 256)

    def slots(n):
        s = 1024
        while s < 2 * n:
            s *= 2
        return s

    for V, F in ((0, 0), (1, 1), (5, 0), (0, 5), (257, 1023), (512, 513), (78302, 152882), (1 << 20, (1 << 21) + 3),
                 (2 ** 31 - 1, 2 ** 31 - 1)):
        want = 64 + pad(4 * tiles(V)) + pad(4 * tiles(F)) + 3 * pad(4 * V) + pad(4 * F) + 64 * slots(V) + 4 * slots(F)
        assert L.m3_mesh_simplify_ws_bytes(V, F) == want == simplify.workspace_bytes(V, F), (V, F)
        assert slots(V) >= 2 * V and slots(F) >= 2 * F                           # at most half full
    for V, F in ((-1, 4), (4, -1), (2 ** 31, 4), (4, 2 ** 31)):
        assert L.m3_mesh_simplify_ws_bytes(V, F) == 0, (V, F)
        with pytest.raises(ValueError):
            simplify.workspace_bytes(V, F)
    one, big = 0x1000, 1 << 40                                                  # never dereferenced: every call below is refused
    nan, inf = float("nan"), float("inf")
    for n in ("m3_mesh_simplify_count", "m3_mesh_simplify_scatter"):            # the prototypes of the header on the raw handle
        getattr(built_lib, n).argtypes, getattr(built_lib, n).restype = getattr(L, n).argtypes, getattr(L, n).restype
    count = lambda **k: built_lib.m3_mesh_simplify_count(*[k.get(n, d) for n, d in (
        ("vertices", one), ("colors", one), ("faces", one), ("V", 8), ("F", 8), ("voxel", 0.5), ("ws", one), ("ws_bytes", big),
        ("stream", None))])
    for bad in (dict(vertices=None), dict(colors=None), dict(faces=None), dict(ws=None), dict(V=-1), dict(F=-1), dict(V=2 ** 31),
                dict(F=2 ** 31), dict(ws=one + 8), dict(ws_bytes=L.m3_mesh_simplify_ws_bytes(8, 8) - 1), dict(vertices=one + 2),
                dict(faces=one + 1), dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=nan), dict(voxel=inf)):
        assert count(**bad) == -1, bad
    scatter = lambda **k: built_lib.m3_mesh_simplify_scatter(*[k.get(n, d) for n, d in (
        ("vertices", one), ("colors", one), ("faces", one), ("V", 8), ("F", 8), ("ws", one), ("ws_bytes", big), ("V2", 4), ("F2", 4),
        ("vout", one), ("cout", one), ("fout", one), ("cluster_of", None), ("frows", None), ("stream", None))])
    for bad in (dict(vertices=None), dict(colors=None), dict(faces=None), dict(ws=None), dict(vout=None), dict(cout=None),
                dict(fout=None), dict(V=-1), dict(F=2 ** 31), dict(V2=-1), dict(F2=-1), dict(V2=9), dict(F2=9), dict(ws=one + 8),
                dict(ws_bytes=64), dict(cluster_of=one + 4), dict(frows=one + 4), dict(vertices=one + 2), dict(fout=one + 2)):
        assert scatter(**bad) == -1, bad
