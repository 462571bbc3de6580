"""CPU: the mesh-components rule (tests/components_twin.py) against closed forms and a pure-Python breadth-first search,
the tie and min_fraction rules, the host checks of mast3r_slam/components.py that need no device, and the workspace
size, launch count and argument validation of the C entry points, which happen before any HIP call."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import components_twin as CC
from mast3r_slam import _ffi, components, mast3r_utils


# ---- the twin --------------------------------------------------------------------------------------------------------
def test_closed_forms():
    for order in ("ascending", "descending", "shuffled"):
        v, c, f = CC.strip(50, order, seed=3)
        lab, of, info, invalid = CC.components(f, v.shape[0])
        assert not lab.any() and (of == 50).all() and info == (1, 50, 0) and invalid == 0      # one component, label = row 0
    k = 9
    f = CC.strip_faces(1, 0)
    f = np.concatenate([f + 3 * i for i in range(k)])
    lab, of, info, _ = CC.components(f, 3 * k + 2)                                  # k disjoint triangles, two loose vertices
    assert np.array_equal(lab, np.r_[np.repeat(3 * np.arange(k), 3), 3 * k, 3 * k + 1]) and info == (k, 1, 0)
    assert np.array_equal(of, np.r_[np.ones(3 * k), 0, 0])
    # fans: one shared row joins them, a twin row at the same coordinates does not
    v, c, f = CC.fans(False)
    assert CC.components(f, v.shape[0])[2] == (1, 14, 0)
    v, c, f = CC.fans(True)
    lab, of, info, _ = CC.components(f, v.shape[0])
    assert info == (2, 7, 0) and lab[8] == 0 and lab[-1] == 9 and v[8].tobytes() == v[-1].tobytes()
    # a face that names a row twice connects and counts; an invalid face connects nothing, is counted and never kept
    f = np.array([[0, 0, 1], [2, 3, 3], [1, 2, 2], [4, 5, 6], [4, 5, 7], [6, 7, -1]], dtype=np.int32)
    lab, of, info, invalid = CC.components(f, 7)
    assert lab.tolist() == [0, 0, 0, 0, 4, 4, 4] and of.tolist() == [3, 3, 3, 3, 1, 1, 1] and info == (2, 3, 0) and invalid == 2
    with pytest.raises(ValueError):
        CC.filter_mesh(*CC.arrays(7, 0), f)
    # nothing at all
    lab, of, info, invalid = CC.components(np.zeros((0, 3), dtype=np.int32), 0)
    assert lab.shape == (0,) and info == (0, 0, -1)
    assert CC.components(np.zeros((0, 3), dtype=np.int32), 3)[2] == (0, 0, -1)


def test_twin_against_breadth_first_search():
    rng = np.random.default_rng(17)
    for trial in range(60):
        V = int(rng.integers(1, 40))
        F = int(rng.integers(0, 30))
        f = rng.integers(-1 if trial % 5 == 0 else 0, V + (1 if trial % 5 == 0 else 0), (F, 3)).astype(np.int32)
        lab = CC.labels_of(f, V)
        assert np.array_equal(lab, CC.bfs_labels(f, V)), trial
        ok = CC.valid_faces(f, V)
        want = np.bincount(lab[f[ok, 0]], minlength=V)[lab]
        assert np.array_equal(CC.components(f, V)[1], want)
    for mesh in (CC.islands(40, (2, 5, 5)), CC.strip(300, "shuffled", 4), CC.with_unreferenced(CC.fans(False), [0, 5, 17])):
        assert np.array_equal(CC.labels_of(mesh[2], mesh[0].shape[0]), CC.bfs_labels(mesh[2], mesh[0].shape[0]))


def test_tie_goes_to_the_smaller_label():
    v, c, f = CC.islands(20, (4, 6, 6, 6), seed=2)
    lab, of, info, _ = CC.components(f, v.shape[0])
    roots = np.flatnonzero((lab == np.arange(v.shape[0])) & (of == 6))
    assert roots.shape[0] == 3 and info.largest == 6 and info.winner == roots.min()
    v2, c2, f2, rows_v, rows_f = CC.filter_mesh(v, c, f, largest_only=True)
    assert f2.shape[0] == 6 and v2.shape[0] == 8 and (lab[rows_v] == roots.min()).all()
    assert np.array_equal(rows_v[f2], f[rows_f]) and v2.tobytes() == v[rows_v].tobytes()
    assert (np.diff(rows_v) > 0).all() and (np.diff(rows_f) > 0).all()


def sizes_kept(mesh, **kw):
    out = CC.filter_mesh(*mesh, **kw)
    lab, of, _, _ = CC.components(mesh[2], mesh[0].shape[0])
    return sorted(set(of[out[3]].tolist()))


def test_min_fraction_is_one_double_multiply_and_compare():
    mesh = CC.islands(10, (5, 12, 13, 40))
    # fp32(0.3) = 0.300000011920929: times 40 it is 12.0000004768, not an integer: 12 faces fail, 13 pass
    assert float(np.float64(np.float32(0.3)) * 40.0) > 12.0
    assert sizes_kept(mesh, min_fraction=0.3) == [13, 40]
    # 0.125 * 40 is exactly 5: 5 faces pass; the next fp32 above 0.125 fails them
    assert sizes_kept(mesh, min_fraction=0.125) == [5, 12, 13, 40]
    assert sizes_kept(mesh, min_fraction=np.nextafter(np.float32(0.125), np.float32(1))) == [12, 13, 40]
    assert sizes_kept(mesh, min_fraction=0.0) == [1, 5, 12, 13, 40] == sizes_kept(mesh, min_faces=-3)
    assert sizes_kept(mesh, min_fraction=1.0) == [40] and sizes_kept(mesh, min_faces=13, min_fraction=0.125) == [13, 40]
    assert sizes_kept(mesh, min_faces=41) == []


# ---- host checks -----------------------------------------------------------------------------------------------------
def test_cpu_tensors_and_bad_arguments():
    v, c, f = (torch.from_numpy(a) for a in CC.fans(False))
    with pytest.raises(RuntimeError, match="ROCm device"):
        components.mesh_components(f, v.shape[0])
    with pytest.raises(RuntimeError, match="ROCm device"):
        components.filter_components(v, c, f)
    with pytest.raises(RuntimeError, match="ROCm device"):
        components.filter_components((v, c, f), largest_only=True)
    for kw in (dict(min_fraction=-0.1), dict(min_fraction=1.5), dict(min_fraction=float("nan")), dict(min_faces=2.5),
               dict(min_faces=True)):
        with pytest.raises(ValueError):
            components.filter_components(v, c, f, **kw)
    with pytest.raises(ValueError):
        components.filter_components(v, c[:-1], f)
    with pytest.raises(ValueError):
        components.filter_components(v, c, f.to(torch.int64))
    with pytest.raises(ValueError):
        components.filter_components((v, c, f), c, f)
    with pytest.raises(ValueError):
        components.mesh_components(f, -1)
    with pytest.raises(ValueError):
        components.mesh_components(f.reshape(-1), 10)


def test_re_exports_and_signatures():
    for n in ("mesh_components", "filter_components", "ComponentsInfo"):
        assert n in mast3r_utils.__all__ and n in components.__all__ and getattr(mast3r_utils, n) is getattr(components, n)
    E = inspect.Parameter.empty
    sig = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    assert sig(components.mesh_components) == [("faces", E), ("n_vertices", E), ("workspace", None)]
    assert sig(components.filter_components) == [("vertices", E), ("colors", None), ("faces", None), ("min_faces", 1),
                                                 ("min_fraction", 0.0), ("largest_only", False), ("return_index", False),
                                                 ("workspace", None)]
    assert components.ComponentsInfo._fields == ("components", "largest", "winner")


def test_symbols_workspace_launches_and_argument_validation():
    names = [n for n in _ffi.declared_symbols() if n.startswith("m3_mesh_components")]
    assert sorted(names) == ["m3_mesh_components_count", "m3_mesh_components_label", "m3_mesh_components_launches",
                             "m3_mesh_components_scatter", "m3_mesh_components_ws_bytes"]
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), n
    L = _ffi.lib()
    assert L.m3_abi_version() == 4000
    assert L.m3_mesh_components_launches() == 11                                # 6 to label, 3 to count, 2 to scatter
    # 64 bytes of header, an int32 offset per tile of 256 vertices and of 256 faces, four int32 arrays of V rows; every
    # array padded to 16 bytes
    pad = lambda b: (b + 15) // 16 * 16
    for V, F in ((0, 0), (1, 1), (5, 0), (0, 5), (257, 1023), (78302, 152882), (1 << 20, (1 << 21) + 3), (2 ** 31 - 1, 2 ** 31 - 1)):
        want = 64 + pad(4 * ((V + 255) // 256)) + pad(4 * ((F + 255) // 256)) + 4 * pad(4 * V)
        assert L.m3_mesh_components_ws_bytes(V, F) == want == components.workspace_bytes(V, F), (V, F)
    for V, F in ((-1, 4), (4, -1), (2 ** 31, 4), (4, 2 ** 31)):
        assert L.m3_mesh_components_ws_bytes(V, F) == 0, (V, F)
        with pytest.raises(ValueError):
            components.workspace_bytes(V, F)
    one, big = 0x1000, 1 << 40                                                  # never dereferenced: every call below is refused
    label = lambda **k: L.m3_mesh_components_label(*[k.get(n, d) for n, d in (
        ("faces", one), ("V", 8), ("F", 8), ("ws", one), ("ws_bytes", big), ("labels", one), ("faces_of", one), ("stream", None))])
    for bad in (dict(faces=None), dict(ws=None), dict(V=-1), dict(F=-1), dict(V=2 ** 31), dict(F=2 ** 31), dict(ws=one + 8),
                dict(ws_bytes=L.m3_mesh_components_ws_bytes(8, 8) - 1), dict(faces=one + 2), dict(labels=one + 1)):
        assert label(**bad) == -1, bad
    nan = float("nan")
    count = lambda **k: L.m3_mesh_components_count(*[k.get(n, d) for n, d in (
        ("ws", one), ("V", 8), ("F", 8), ("faces", one), ("min_faces", 1), ("min_fraction", 0.0), ("largest_only", 0), ("stream", None))])
    for bad in (dict(ws=None), dict(faces=None), dict(V=-1), dict(F=2 ** 31), dict(min_fraction=-0.5), dict(min_fraction=1.5),
                dict(min_fraction=nan), dict(largest_only=2), dict(ws=one + 4)):
        assert count(**bad) == -1, bad
    scatter = lambda **k: L.m3_mesh_components_scatter(*[k.get(n, d) for n, d in (
        ("vertices", one), ("colors", one), ("faces", one), ("V", 8), ("F", 8), ("ws", one), ("V2", 4), ("F2", 4), ("vout", one),
        ("cout", one), ("fout", one), ("vrows", None), ("frows", None), ("stream", None))])
    for bad in (dict(vertices=None), dict(colors=None), dict(faces=None), dict(ws=None), dict(vout=None), dict(cout=None),
                dict(fout=None), dict(V=-1), dict(V2=0), dict(F2=0), dict(V2=9), dict(F2=9), dict(ws=one + 8), dict(vrows=one + 4),
                dict(vertices=one + 2)):
        assert scatter(**bad) == -1, bad
