"""CPU: the point-cloud neighbourhood rule (tests/cloud_twin.py) against things that do not come from the twin - a
brute-force float64 distance matrix, the count of an integer lattice, a five-point case written out by hand; the host
checks of mast3r_slam/cloud.py that need no device; the PLY writer for clouds with normals; and the workspace size,
launch count and argument validation of the C entry points, which happen before any HIP call."""
import ctypes
import inspect
import os
import types

import numpy as np
import pytest
import torch

import cloud_twin as CT
from mast3r_slam import _ffi, cloud, export, mast3r_utils


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
@pytest.mark.parametrize("scene", sorted(CT.SCENES))
def test_counts_against_a_distance_matrix(scene):
    p, r = CT.SCENES[scene]()
    assert p.dtype == np.float32 and len(p) <= 4100
    got = CT.neighbors(p, r)
    assert got["out_of_range"] == 0
    assert np.array_equal(got["count"], CT.brute_counts(p, r))
    finite = np.isfinite(p).all(axis=1)
    assert (got["count"][finite] >= 1).all() and (got["count"][~finite] == 0).all() and (got["moments"][~finite] == 0).all()
    for i in np.flatnonzero(finite)[:50]:
        assert i in got["sets"][i]                                              # a point is its own neighbour


def test_lattice_counts_need_no_twin():
    """Spacing 1/8 at r = 1/8: the six axis neighbours lie exactly on the boundary, the diagonal ones outside."""
    p, r = CT.lattice()
    inner = CT.lattice_interior()
    assert len(p) == 3 * 9 ** 3 and inner.sum() == 3 * 7 ** 3
    assert (CT.neighbors(p, r)["count"][inner] == 7).all()
    assert np.abs(p[:, 0]).max() > 128 and np.abs(p[:, 1]).max() > 256         # the copy across the powers of two
    c = CT.cells(p, r)
    assert len(np.unique(c[:, 0])) > 9 and (np.abs(c) < 2 ** 20).all()
    # at the diagonal radius the twelve face diagonals are within rounding of the boundary: in or out together
    p, r = CT.lattice_diagonal()
    n = CT.neighbors(p, r)["count"][inner]
    assert n.min() == n.max() and n[0] in (7, 19)


def test_five_points_by_hand():
    p = np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.25, 0], [0, 0, -1], [2, 0, 0]], np.float32)
    got = CT.neighbors(p, 1.0)                                                  # scale = 2^20
    assert got["count"].tolist() == [4, 3, 3, 2, 1]
    # point 0 sees 1, 2 and - exactly on the boundary - 3: offsets (2^19,0,0), (0,2^18,0), (0,0,-2^20)
    assert got["moments"][0].tolist() == [2 ** 19, 2 ** 18, -2 ** 20, 2 ** 38, 0, 0, 2 ** 36, 0, 2 ** 40]
    # point 1 sees 0 (-2^19,0,0) and 2 (-2^19,2^18,0)
    assert got["moments"][1].tolist() == [-2 ** 20, 2 ** 18, 0, 2 ** 39, -2 ** 37, 0, 2 ** 36, 0, 0]
    # point 3 sees 0 alone, at (0,0,2^20); point 4 only itself
    assert got["moments"][3].tolist() == [0, 0, 2 ** 20, 0, 0, 0, 0, 0, 2 ** 40]
    assert got["moments"][4].tolist() == [0] * 9
    C = CT.covariance(got["count"], got["moments"])
    assert C[3].tolist() == [[0, 0, 0], [0, 0, 0], [0, 0, 2.0 ** 40 / 2 - 2.0 ** 40 / 4]]
    assert CT.judged(got["count"], got["moments"]).tolist() == [True, True, True, False, False]
    assert CT.kept_rows(p, 1.0, 2).tolist() == [0, 1, 2] and CT.kept_rows(p, 1.0, 0).tolist() == [0, 1, 2, 3, 4]


def test_rounding_range_and_points_that_are_not_finite():
    p = np.array([[0, 0, 0], [1.5 / 2 ** 20, 0, 0], [2.5 / 2 ** 20, 0, 0], [0, -3.5 / 2 ** 20, 0]], np.float32)
    got = CT.neighbors(p, 1.0)                                                  # scale = 2^20: the products are exact
    assert got["moments"][0].tolist() == [2 + 2, -4, 0, 4 + 4, 0, 0, 16, 0, 0]    # half to even, as the rule says
    r = 3.0
    far = np.array([[0, 0, 0], [3.1 * 2 ** 20, 0, 0], [np.nan, 0, 0], [0, -3.1 * 2 ** 20, 0]], np.float32)
    got = CT.neighbors(far, r)
    assert got["out_of_range"] == 2 and got["count"].tolist() == [1, 0, 0, 0]
    assert CT.neighbors(far[:1] + np.float32(2.9 * 2 ** 20), r)["out_of_range"] == 0


def test_floaters_scene_is_what_the_filter_test_needs():
    p, r = CT.floaters()
    rows = CT.floaters_rows()
    count = CT.neighbors(p, r)["count"]
    assert rows["isolated"].sum() == 50 and rows["duplicate"].sum() == 20 and rows["bad"].sum() == 3
    assert (count[rows["isolated"]] == 1).all() and (count[rows["bad"]] == 0).all() and (count[rows["duplicate"]] >= 3).all()
    gone = np.ones(len(p), bool)
    gone[CT.kept_rows(p, r, 2, count)] = False
    assert np.array_equal(gone, rows["isolated"] | rows["bad"])
    assert np.array_equal(CT.kept_rows(p, r, 0, count), np.flatnonzero(~rows["bad"]))
    assert len(CT.kept_rows(p, r, 4000, count)) == 0


# ---- host checks -----------------------------------------------------------------------------------------------------
def test_cpu_tensors_and_bad_arguments(monkeypatch):
    p = torch.from_numpy(CT.plane()[0])
    c = torch.zeros((len(p), 3), dtype=torch.uint8)
    idx = torch.arange(len(p))
    # arguments that cannot be used are refused before the library is needed
    monkeypatch.setattr(_ffi, "lib", lambda: pytest.fail("the library was loaded"))
    nan, inf = float("nan"), float("inf")
    for r in (0.0, -1.0, nan, inf, 1e-60, 1e60, None, "1", True):
        with pytest.raises(ValueError):
            cloud.cloud_neighbors(p, r)
        with pytest.raises(ValueError):
            cloud.cloud_normals(p, r)
        with pytest.raises(ValueError):
            cloud.remove_radius_outliers(p, c, radius=r, min_neighbors=2)
    for bad in (p.double(), p.reshape(-1), p[:, :2], p.numpy(), None):
        with pytest.raises(ValueError):
            cloud.cloud_neighbors(bad, 0.05)
        with pytest.raises(ValueError):
            cloud.cloud_normals(bad, 0.05)
        with pytest.raises(ValueError):
            cloud.remove_radius_outliers(bad, c, radius=0.05, min_neighbors=2)
    for kw in (dict(min_points=0), dict(min_points=2.5), dict(min_points=None), dict(toward=torch.zeros(4)),
               dict(toward=torch.zeros((len(p) - 1, 3))), dict(toward=torch.zeros(3, dtype=torch.float64)), dict(toward=np.zeros(3))):
        with pytest.raises(ValueError):
            cloud.cloud_normals(p, 0.05, **kw)
    with pytest.raises(ValueError):
        cloud.cloud_normals((p,), 0.05)
    for args, kw in (((p, c), dict(radius=0.05)), ((p, c), dict(min_neighbors=2)), ((p, c), dict(radius=0.05, min_neighbors=-1)),
                     ((p, c), dict(radius=0.05, min_neighbors=1.5)), ((p, c[:-1]), dict(radius=0.05, min_neighbors=2)),
                     ((p, None), dict(radius=0.05, min_neighbors=2)), ((p, c.float()), dict(radius=0.05, min_neighbors=2)),
                     ((p, c, idx[:-1]), dict(radius=0.05, min_neighbors=2)), ((p, c, idx.int()), dict(radius=0.05, min_neighbors=2)),
                     (((p, c), c), dict(radius=0.05, min_neighbors=2)), (((p, c, idx, idx),), dict(radius=0.05, min_neighbors=2)),
                     (((p,),), dict(radius=0.05, min_neighbors=2))):
        with pytest.raises(ValueError):
            cloud.remove_radius_outliers(*args, **kw)
    for call in (lambda: cloud.cloud_neighbors(p, 0.05), lambda: cloud.cloud_neighbors(p, 0.05, moments=False),
                 lambda: cloud.cloud_normals(p, 0.05), lambda: cloud.cloud_normals((p, c, idx), 0.05, toward=torch.zeros(3)),
                 lambda: cloud.remove_radius_outliers(p, c, radius=0.05, min_neighbors=2),
                 lambda: cloud.remove_radius_outliers((p, c, idx), radius=0.05, min_neighbors=2, return_rows=True)):
        with pytest.raises(RuntimeError, match="ROCm device"):
            call()


def test_source_viewpoints_is_plain_indexing():
    n = 6
    frames = [types.SimpleNamespace(X_canon=torch.zeros((n, 3)), T_WC=torch.tensor([[10.0 * k, 1.0, -k, 0, 0, 0, 1, 1.5]]))
              for k in range(3)]
    frames.insert(1, types.SimpleNamespace(X_canon=None, T_WC=torch.full((1, 8), 99.0)))     # no pointmap: skipped
    idx = torch.tensor([0, 5, 6, 17, 12], dtype=torch.int64)
    got = cloud.source_viewpoints(frames, idx)
    assert got.dtype == torch.float32 and got.tolist() == [[0, 1, 0], [0, 1, 0], [10, 1, -1], [20, 1, -2], [20, 1, -2]]
    assert cloud.source_viewpoints(types.SimpleNamespace(_frames=frames), idx).tolist() == got.tolist()
    assert tuple(cloud.source_viewpoints(frames, idx[:0]).shape) == (0, 3)
    for bad in (idx.int(), idx.reshape(-1, 1), idx.numpy(), torch.tensor([18]), torch.tensor([-1])):
        with pytest.raises(ValueError):
            cloud.source_viewpoints(frames, bad)
    with pytest.raises(ValueError):
        cloud.source_viewpoints([], idx)


def test_re_exports_and_signatures():
    for n in ("cloud_neighbors", "cloud_normals", "source_viewpoints", "remove_radius_outliers", "CloudNeighbors"):
        assert n in mast3r_utils.__all__ and n in cloud.__all__ and getattr(mast3r_utils, n) is getattr(cloud, n)
    assert "save_ply_normals" in mast3r_utils.__all__ and "save_ply_normals" in export.__all__
    assert mast3r_utils.save_ply_normals is export.save_ply_normals and "workspace_bytes" in cloud.__all__
    E = inspect.Parameter.empty
    sig = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    assert sig(cloud.cloud_neighbors) == [("points", E), ("radius", E), ("moments", True), ("workspace", None)]
    assert sig(cloud.cloud_normals) == [("points", E), ("radius", E), ("toward", None), ("min_points", 3), ("return_variation", False),
                                        ("workspace", None)]
    assert sig(cloud.source_viewpoints) == [("keyframes", E), ("index", E)]
    assert [n for n, _ in sig(cloud.remove_radius_outliers)] == ["points", "colors", "index", "radius", "min_neighbors", "return_rows"]
    assert sig(cloud.workspace_bytes) == [("M", E)]
    assert sig(export.save_ply_normals) == [("path", E), ("points", E), ("colors", E), ("normals", E), ("binary", True)]
    assert cloud.CloudNeighbors._fields == ("count", "moments", "out_of_range")


# ---- the PLY writer --------------------------------------------------------------------------------------------------
def parse_header(path):
    with open(path, "rb") as f:
        lines = []
        while True:
            line = f.readline().decode("ascii").strip()
            lines.append(line)
            if line == "end_header":
                return lines, f.tell()


@pytest.mark.parametrize("binary", [True, False])
def test_save_ply_normals_round_trips(tmp_path, binary):
    g = np.random.default_rng(5)
    p = g.normal(size=(37, 3)).astype(np.float32)
    n = g.normal(size=(37, 3)).astype(np.float32)
    c = g.integers(0, 256, size=(37, 3), dtype=np.uint8)
    path = tmp_path / "cloud.ply"
    assert export.save_ply_normals(path, torch.from_numpy(p), torch.from_numpy(c), torch.from_numpy(n), binary=binary) == 37
    lines, at = parse_header(path)
    assert lines[:3] == ["ply", f"format {'binary_little_endian' if binary else 'ascii'} 1.0", "element vertex 37"]
    assert lines[3:-1] == [f"property float {a}" for a in ("x", "y", "z", "nx", "ny", "nz")] + \
        [f"property uchar {a}" for a in ("red", "green", "blue")]               # and no face element
    if binary:
        body = np.fromfile(path, dtype=export._PLY_NORMALS_DTYPE, offset=at)
        assert body.shape == (37,) and os.path.getsize(path) == at + 37 * 27
        assert np.stack([body["x"], body["y"], body["z"]], axis=1).tobytes() == p.tobytes()
        assert np.stack([body["nx"], body["ny"], body["nz"]], axis=1).tobytes() == n.tobytes()
        assert np.stack([body["red"], body["green"], body["blue"]], axis=1).tobytes() == c.tobytes()
    else:
        body = np.loadtxt(path, skiprows=len(lines)).reshape(-1, 9)
        assert body.shape == (37, 9) and np.abs(body[:, :3] - p).max() <= 5.1e-7 and np.abs(body[:, 3:6] - n).max() <= 5.1e-7
        assert np.array_equal(body[:, 6:], c)
    assert export.save_ply_normals(path, p[:0], c[:0], n[:0], binary=binary) == 0
    assert parse_header(path)[0][2] == "element vertex 0" and os.path.getsize(path) == parse_header(path)[1]
    for args in ((p, c[:-1], n), (p, c, n[:-1])):
        with pytest.raises(ValueError):
            export.save_ply_normals(path, *args)


# ---- the C entry points ----------------------------------------------------------------------------------------------
def test_symbols_workspace_launches_and_argument_validation(built_lib):
    names = [n for n in _ffi.declared_symbols() if n.startswith("m3_cloud_")]
    assert sorted(names) == ["m3_cloud_launches", "m3_cloud_neighbors", "m3_cloud_normals", "m3_cloud_radius_count",
                             "m3_cloud_radius_scatter", "m3_cloud_ws_bytes"]
    for n in names:
        assert hasattr(built_lib, n), n
    L = _ffi.lib()
    assert L.m3_cloud_launches() == 7
    pad = lambda b: (b + 15) // 16 * 16

    def slots(n):
        s = 1024
        while s < n:
            s *= 2
        return s

    for M in (0, 1, 5, 511, 512, 513, 1025, 4000, 78302, (1 << 20) + 3, 2 ** 30):
        S = slots(2 * M)
        want = 64 + pad(4 * ((S + 1 + 255) // 256)) + pad(4 * (S + 1)) + 8 * S + 3 * pad(4 * M) + 16 * M
        assert L.m3_cloud_ws_bytes(M) == want == cloud.workspace_bytes(M), M
        assert (M + 1023) // 1024 <= (S + 1 + 255) // 256                       # the filter's tile offsets fit the tile array
    for M in (-1, 2 ** 30 + 1, 2 ** 40):
        assert L.m3_cloud_ws_bytes(M) == 0, M
        with pytest.raises(ValueError):
            cloud.workspace_bytes(M)
    one, big = 0x1000, 1 << 40                                                  # never dereferenced: every call below is refused
    nan, inf = float("nan"), float("inf")
    for n in names:                                                             # the prototypes of the header on the raw handle
        getattr(built_lib, n).argtypes, getattr(built_lib, n).restype = getattr(L, n).argtypes, getattr(L, n).restype
    short = L.m3_cloud_ws_bytes(8) - 1
    nb = lambda **k: built_lib.m3_cloud_neighbors(*[k.get(n, d) for n, d in (
        ("points", one), ("M", 8), ("radius", 0.5), ("scale", 2.0 ** 21), ("count", one), ("moments", one), ("ws", one),
        ("ws_bytes", big), ("stream", None))])
    for bad in (dict(points=None), dict(count=None), dict(ws=None), dict(M=-1), dict(M=2 ** 30 + 1), dict(ws=one + 8),
                dict(ws_bytes=short), dict(points=one + 2), dict(count=one + 2), dict(moments=one + 4), dict(radius=0.0),
                dict(radius=-1.0), dict(radius=nan), dict(radius=inf), dict(scale=0.0), dict(scale=-1.0), dict(scale=nan),
                dict(scale=inf), dict(scale=2.0 ** 23)):
        assert nb(**bad) == -1, bad
    nm = lambda **k: built_lib.m3_cloud_normals(*[k.get(n, d) for n, d in (
        ("points", one), ("M", 8), ("count", one), ("moments", one), ("toward", one), ("stride", 3), ("min_points", 3),
        ("normals", one), ("variation", one), ("stream", None))])
    for bad in (dict(points=None), dict(count=None), dict(moments=None), dict(normals=None), dict(M=-1), dict(M=2 ** 30 + 1),
                dict(stride=1), dict(stride=-3), dict(min_points=0), dict(min_points=-1), dict(points=one + 2), dict(count=one + 1),
                dict(moments=one + 4), dict(toward=one + 2), dict(normals=one + 2), dict(variation=one + 2)):
        assert nm(**bad) == -1, bad
    rc = lambda **k: built_lib.m3_cloud_radius_count(*[k.get(n, d) for n, d in (
        ("count", one), ("M", 8), ("min_neighbors", 2), ("ws", one), ("ws_bytes", big), ("stream", None))])
    for bad in (dict(count=None), dict(ws=None), dict(M=-1), dict(M=2 ** 30 + 1), dict(min_neighbors=-1), dict(ws=one + 4),
                dict(ws_bytes=short), dict(count=one + 2)):
        assert rc(**bad) == -1, bad
    rs = lambda **k: built_lib.m3_cloud_radius_scatter(*[k.get(n, d) for n, d in (
        ("points", one), ("colors", one), ("index", one), ("count", one), ("M", 8), ("min_neighbors", 2), ("ws", one),
        ("ws_bytes", big), ("M2", 4), ("points_out", one), ("colors_out", one), ("index_out", one), ("rows_out", one),
        ("stream", None))])
    for bad in (dict(points=None), dict(count=None), dict(ws=None), dict(points_out=None), dict(M=-1), dict(M2=-1), dict(M2=9),
                dict(min_neighbors=-1), dict(ws=one + 8), dict(ws_bytes=short), dict(colors=None), dict(colors_out=None),
                dict(index_out=None), dict(points=one + 2), dict(index=one + 4), dict(index_out=one + 4), dict(rows_out=one + 4),
                dict(points_out=one + 1)):
        assert rs(**bad) == -1, bad
