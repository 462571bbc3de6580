"""Host side of the vertex normals: the twin (tests/normals_twin.py) against analytic normals and against itself in
float64, the shading twin, the C entry points' argument checks, the PLY writer with normals, and the Python checks
that need no device.

Float32 rule against the float64 twin (same equal-weight rule, no quantisation) on the wavy sheet of normals_twin.sheet,
largest difference of one component: 5.21e-8 at 17x13 (221 vertices, 384 faces), 5.44e-8 at 129x97 (12 513 vertices,
24 576 faces), 6.43e-8 at 513x385 (197 505 vertices, 393 216 faces).  The bound below is 4 x the largest of them."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import normals_twin as NT
from mast3r_slam import _ffi, export, mast3r_utils, normals, render

TWIN_ERROR = 6.43e-8                                                        # measured: see the docstring
SHEETS = ((17, 13, 221, 384), (129, 97, 12513, 24576), (513, 385, 197505, 393216))


# ---- the twin against closed forms -----------------------------------------------------------------------------------
def test_plane_and_cube_are_exact():
    V, F = NT.sheet(9, 7, lambda X, Y: 2.0 + 0.0 * X)
    n = NT.vertex_normals(V, F)
    assert n.dtype == np.float32 and np.array_equal(n, np.broadcast_to(np.float32([0, 0, -1]), n.shape))   # faces the camera at -z
    assert np.array_equal(NT.vertex_normals(V, F[:, [0, 2, 1]]), -n)
    V, F = NT.cube_with_centres()
    n = NT.vertex_normals(V, F)
    assert np.array_equal(n[8:], V[8:])                                         # the six face centres: the axes, exactly
    want = V[:8] / np.sqrt(np.float32(3))                                       # a corner: three faces' worth of each axis
    assert np.abs(n[:8] - want).max() < 1e-7
    assert np.array_equal(NT.vertex_sums(V, F)[8:], (4 << 24) * V[8:].astype(np.int64))


def test_sphere_within_the_angle_of_its_facets():
    for levels in (2, 3, 4):
        V, F = NT.sphere(levels)
        assert len(F) == 8 * 4 ** levels and len(V) == len(F) // 2 + 2          # closed: Euler's formula
        P = V.astype(np.float64)
        a, b, c = P[F[:, 0]], P[F[:, 1]], P[F[:, 2]]
        ea, eb, ec = (np.linalg.norm(x, axis=1) for x in (b - c, c - a, a - b))
        area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
        # a facet's plane normal passes through its circumcentre, at asin(circumradius) from each of its corners on the
        # unit sphere; a vertex normal is a mean of unit vectors inside that cone around the vertex
        bound = float(np.arcsin((ea * eb * ec / (4 * area)).max())) + 1e-6
        for n in (NT.vertex_normals(V, F).astype(np.float64), NT.vertex_normals64(V, F)):
            assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 2e-7
            angle = np.arccos(np.clip((n * P).sum(axis=1) / np.linalg.norm(P, axis=1), -1, 1))
            print(f"levels {levels}: largest angle {angle.max():.5f}, bound {bound:.5f}")
            assert angle.max() <= bound


@pytest.mark.parametrize("nx,ny,nv,nf", SHEETS)
def test_float32_rule_against_the_float64_twin(nx, ny, nv, nf):
    V, F = NT.sheet(nx, ny)
    assert (len(V), len(F)) == (nv, nf)
    n32, n64 = NT.vertex_normals(V, F), NT.vertex_normals64(V, F)
    err = float(np.abs(n32.astype(np.float64) - n64).max())
    print(f"{nx}x{ny}: {err:.3e}")
    assert err <= 4 * TWIN_ERROR
    assert NT.vertex_normals(V, NT.permuted(F, 1)).tobytes() == n32.tobytes()  # what the integers buy
    assert np.array_equal(NT.vertex_sums(V, NT.permuted(F, 2)), NT.vertex_sums(V, F))


def test_degenerate_and_out_of_range_faces_give_zero():
    V, F, zero = NT.degenerate()
    n = NT.vertex_normals(V, F)
    assert not n[zero].any() and np.isfinite(n).all()
    rest = np.setdiff1d(np.arange(len(V)), zero)
    assert np.abs(np.linalg.norm(n[rest].astype(np.float64), axis=1) - 1).max() < 2e-7
    good = F[NT.valid_faces(F, len(V)) & (F < zero[0]).all(axis=1) & (F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2])]
    assert NT.vertex_normals(V, good).tobytes() == n.tobytes()                # the bad faces changed nothing
    assert not NT.vertex_normals(V, np.zeros((0, 3), dtype=np.int32)).any()
    assert NT.vertex_normals(np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int32)).shape == (0, 3)


# ---- the shading twin ---------------------------------------------------------------------------------------------------
def test_shade_twin():
    P = np.float32([[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 2]])
    N = np.float32([[0, 0, 1], [0, 0, -1], [0, 0, 0], [np.nan, 0, 0], [0, 0, 1]])
    C = np.full((5, 3), 200, dtype=np.uint8)
    eye = np.float32([0, 0, 2])                                                  # in front of rows 0 ... 3, ON row 4
    one = NT.shade(P, N, C, eye=eye, ambient=0.25, two_sided=False)
    assert one[:, 0].tolist() == [200, 50, 50, 50, 50]            # lit; back face, zero normal, NaN and 0 / 0: ambient only
    two = NT.shade(P, N, C, eye=eye, ambient=0.25, two_sided=True)
    assert two[:, 0].tolist() == [200, 200, 50, 50, 50]
    assert NT.shade(P, N, None, light=[0, 0, 3], ambient=0.0, two_sided=False, albedo=(10, 20, 30)).tolist()[:2] == [[10, 20, 30], [0, 0, 0]]
    assert (NT.shade(P, N, C, eye=eye, ambient=1.0) == 200).all()
    grazing = NT.shade(P[:1], N[:1], C[:1], light=[1, 0, 1], ambient=0.0)     # cos 45 degrees
    assert grazing[0, 0] == math.floor(200 * math.sqrt(0.5) + 0.5)
    assert NT.shade(P[:1], np.float32([[0, 0, 1]]), mode="normals").tolist() == [[128, 128, 255]]
    assert NT.shade(P[:3], N[:3], mode="normals").tolist() == [[128, 128, 255], [128, 128, 0], [128, 128, 128]]
    assert NT.shade(P[:1], np.float32([[np.nan, np.inf, -np.inf]]), mode="normals").tolist() == [[0, 255, 0]]
    for dt in (np.float32, np.float64):
        assert NT.shade(P, N, C, eye=eye, dtype=dt).dtype == np.uint8


# ---- entry points ---------------------------------------------------------------------------------------------------------
def test_symbols_workspace_launches_and_argument_validation():
    names = ["m3_mesh_normals", "m3_mesh_normals_launches", "m3_mesh_normals_ws_bytes", "m3_mesh_shade"]
    assert all(n in _ffi.declared_symbols() for n in names)
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), n
    L = _ffi.lib()
    assert L.m3_abi_version() == 4000
    assert L.m3_mesh_normals_launches() == 3                                    # clear, faces, vertices
    for V, want in ((0, 16), (1, 32), (2, 48), (3, 80), (221, 5312), (2 ** 31 - 1, 24 * (2 ** 31 - 1) + 8)):
        assert L.m3_mesh_normals_ws_bytes(V) == want == normals.workspace_bytes(V), V
    for V in (-1, 2 ** 31, 2 ** 40):
        assert L.m3_mesh_normals_ws_bytes(V) == 0
        with pytest.raises(ValueError):
            normals.workspace_bytes(V)
    one, big = 0x1000, 1 << 40                                                  # never dereferenced: every call below is refused
    call = lambda **k: L.m3_mesh_normals(*[k.get(n, d) for n, d in (
        ("vertices", one), ("faces", one), ("V", 8), ("F", 8), ("ws", one), ("ws_bytes", big), ("normals", one), ("stream", None))])
    for bad in (dict(vertices=None), dict(faces=None), dict(normals=None), dict(ws=None), dict(V=-1), dict(F=-1), dict(V=2 ** 31),
                dict(F=2 ** 31), dict(ws=one + 8), dict(ws_bytes=L.m3_mesh_normals_ws_bytes(8) - 1), dict(ws_bytes=0),
                dict(vertices=one + 2), dict(faces=one + 1), dict(normals=one + 2), dict(V=0, F=0, ws=None)):
        assert call(**bad) == -1, bad
    nan, inf = float("nan"), float("inf")
    shade = lambda **k: L.m3_mesh_shade(*[k.get(n, d) for n, d in (
        ("vertices", one), ("normals", one), ("colors", one), ("V", 8), ("view", one), ("light", 0), ("lx", 0.0), ("ly", 0.0),
        ("lz", 1.0), ("ambient", 0.25), ("two_sided", 1), ("mode", 0), ("r", 200), ("g", 200), ("b", 200), ("out", one),
        ("stream", None))])
    for bad in (dict(vertices=None), dict(normals=None), dict(out=None), dict(V=-1), dict(V=2 ** 31), dict(view=None),
                dict(ambient=-0.01), dict(ambient=1.01), dict(ambient=nan), dict(mode=2), dict(mode=-1), dict(light=2),
                dict(two_sided=2), dict(r=256), dict(b=-1), dict(light=1, lz=0.0), dict(light=1, lx=nan), dict(light=1, ly=inf),
                dict(light=1, lz=-inf), dict(normals=one + 2), dict(view=one + 1)):
        assert shade(**bad) == -1, bad


# ---- PLY with normals ------------------------------------------------------------------------------------------------------
def test_ply_with_normals_round_trips(tmp_path):
    V, F = NT.sheet(5, 4)
    N = NT.vertex_normals(V, F)
    C = np.random.default_rng(3).integers(0, 256, size=V.shape).astype(np.uint8)
    assert export.save_ply_mesh_normals(tmp_path / "b.ply", V, C, F, N) == (20, 24)
    pv, pn, pc, pf = NT.read_ply_mesh_normals(tmp_path / "b.ply")
    assert pv.tobytes() == V.tobytes() and pn.tobytes() == N.tobytes() and np.array_equal(pc, C) and np.array_equal(pf, F)
    assert export.save_ply_mesh_normals(tmp_path / "a.ply", *(torch.from_numpy(a) for a in (V, C, F, N)), binary=False) == (20, 24)
    pv, pn, pc, pf = NT.read_ply_mesh_normals(tmp_path / "a.ply")
    assert np.abs(pv - V).max() <= 5e-7 and np.abs(pn - N).max() <= 5e-7 and np.array_equal(pc, C) and np.array_equal(pf, F)
    empty = [np.zeros((0, 3), dtype=d) for d in (np.float32, np.uint8, np.int32, np.float32)]
    for binary in (True, False):
        assert export.save_ply_mesh_normals(tmp_path / "e.ply", *empty, binary=binary) == (0, 0)
        assert all(a.shape == (0, 3) for a in NT.read_ply_mesh_normals(tmp_path / "e.ply"))
    with pytest.raises(ValueError):
        export.save_ply_mesh_normals(tmp_path / "x.ply", V, C, F, N[:-1])
    with pytest.raises(ValueError):
        export.save_ply_mesh_normals(tmp_path / "x.ply", V, C[:-1], F, N)
    with pytest.raises(ValueError):
        export.save_ply_mesh_normals(tmp_path / "x.ply", V, C, F + 1, N)


# ---- Python checks ------------------------------------------------------------------------------------------------------------
def test_re_exports_and_signatures():
    for n in ("vertex_normals", "shade_vertices"):
        assert n in mast3r_utils.__all__ and n in normals.__all__ and getattr(mast3r_utils, n) is getattr(normals, n)
    assert "workspace_bytes" in normals.__all__
    assert "save_ply_mesh_normals" in mast3r_utils.__all__ and mast3r_utils.save_ply_mesh_normals is export.save_ply_mesh_normals
    E = inspect.Parameter.empty
    sig = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    assert sig(normals.vertex_normals) == [("vertices", E), ("faces", None), ("out", None), ("workspace", None)]
    assert sig(normals.shade_vertices) == [("vertices", E), ("normals", E), ("colors", None), ("T_WC", None), ("light", "headlight"),
                                           ("ambient", 0.25), ("two_sided", True), ("mode", "lambert"),
                                           ("albedo", (200, 200, 200)), ("out", None)]
    assert sig(normals.workspace_bytes) == [("n_vertices", E)]
    assert sig(export.save_ply_mesh_normals) == [("path", E), ("vertices", E), ("colors", E), ("faces", E), ("normals", E), ("binary", True)]
    assert sig(export.save_ply_mesh) == [("path", E), ("vertices", E), ("colors", E), ("faces", E), ("binary", True)]
    # render_mesh up to `workspace` is what it was; the three new keywords trail
    assert sig(render.render_mesh) == [("vertices", E), ("colors", None), ("faces", None), ("T_WC", None), ("K", None), ("size", None),
                                       ("near", 1e-3), ("far", math.inf), ("cull", "none"), ("background", (0, 0, 0)),
                                       ("return_index", False), ("out", None), ("workspace", None),
                                       ("shading", None), ("normals", None), ("shade_kw", None)]


def test_cpu_tensors_and_bad_arguments(tmp_path):
    V, F = NT.sheet(5, 4)
    v, f = torch.from_numpy(V), torch.from_numpy(F)
    c, n = torch.zeros(V.shape, dtype=torch.uint8), torch.from_numpy(NT.vertex_normals(V, F))
    pose = torch.tensor([[0, 0, 0, 0, 0, 0, 1, 1]], dtype=torch.float32)
    for args in ((v, f), ((v, c, f),), (v, c, f)):
        with pytest.raises(RuntimeError, match="ROCm device"):
            normals.vertex_normals(*args)
    with pytest.raises(RuntimeError, match="ROCm device"):
        normals.shade_vertices(v, n, c, pose)
    for args in ((v, f.to(torch.int64)), (v.double(), f), (v, f.reshape(-1)), ((v, c),), ((v, c, f), f), (v, c, None), (v, None)):
        with pytest.raises(ValueError):
            normals.vertex_normals(*args)
    for kw in (dict(ambient=-0.1), dict(ambient=1.5), dict(ambient=float("nan")), dict(mode="phong"), dict(light="sun"),
               dict(light=(0, 0, 0)), dict(light=(0, float("nan"), 1)), dict(light=(0, float("inf"), 1)), dict(light=(1, 2)),
               dict(albedo=(0, 0, 256)), dict(albedo=(1, 2)), dict(T_WC=None)):
        with pytest.raises(ValueError):
            normals.shade_vertices(v, n, c, **dict(dict(T_WC=pose), **kw))
    # render_mesh: the new keywords are checked before any tensor is touched
    for kw in (dict(shading="phong"), dict(shading="lambert"), dict(normals=n), dict(shade_kw=dict(ambient=0.5))):
        with pytest.raises(ValueError):
            render.render_mesh(v, c, f, pose, None, (8, 8), **kw)
    # points carry no normals
    with pytest.raises(ValueError, match="shading"):
        render.ViewRecorder(tmp_path / "views", surface="points", shading="headlight")
    render.ViewRecorder(tmp_path / "views", surface="mesh", shading="headlight")
    from mast3r_slam.slam import SLAM
    with pytest.raises(ValueError, match="shading"):
        SLAM.render_view(None, surface="points", shading="headlight")
