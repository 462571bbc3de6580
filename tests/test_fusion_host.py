"""CPU: the two rules of the volumetric fusion (tests/tsdf_twin.py) on a hand-made case whose values are written out, on
an analytic sphere and on every volume the GPU tests use; the host checks of mast3r_slam/fusion.py that need no device;
the workspace sizes and the argument validation of the C entry points, which happens before any HIP call."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import tsdf_twin as TT
from mast3r_slam import _ffi, fusion, mast3r_utils
from mast3r_slam.frame import Frame


# ---- twin self-checks ------------------------------------------------------------------------------------------------
def test_hand_made_case():
    sc, pin, vol, tsdf, weight, color = TT.hand_case()
    for dtype in (np.float64, np.float32):
        tw = TT.integrate(sc, pin, vol, dtype=dtype)
        assert tw["tsdf"].tobytes() == tsdf.tobytes() and np.array_equal(tw["weight"], weight)
        assert np.array_equal(tw["color"], color) and tw["colored"].all() and tw["pairs"].sum() == 0
    one = TT.integrate(dict(sc, X=sc["X"][:1], C=sc["C"][:1], Nk=sc["Nk"][:1], T=sc["T"][:1], img=sc["img"][:1], K=1), pin, vol)
    assert np.array_equal(one["tsdf"], np.array([[[0.5, 0.5], [0.5, 0.5]], [[-0.5, -0.5], [-0.5, -0.5]]], dtype=np.float32))
    assert (one["weight"] == 1).all() and np.array_equal(one["color"][0], sc["img"][0].reshape(2, 2, 3))
    # no threshold: keyframe 1's pixel 3 (depth 2) is an observation too
    free = TT.integrate(sc, pin, vol, thr=None)
    assert free["weight"][:, 1, 1].tolist() == [2, 2] and free["tsdf"][:, 1, 1].tolist() == [0.5, -0.5]
    assert free["color"][0, 1, 1].tolist() == [101, 111, 121]                 # means 100.5, 110.5, 120.5: halves round up
    empty = TT.integrate(dict(sc, X=sc["X"][:0], C=sc["C"][:0], Nk=sc["Nk"][:0], T=sc["T"][:0], img=sc["img"][:0], K=0), pin, vol)
    assert (empty["tsdf"] == 1).all() and not empty["weight"].any() and not empty["color"].any() and not empty["colored"].any()
    # the two layers have opposite signs everywhere but at pixel 2: three of the four z-edges cross, one cell, no face
    v, c, f = TT.extract(tw["tsdf"], tw["weight"], tw["color"], tw["colored"], vol["origin"], vol["vs"])
    assert v.shape == (1, 3) and f.shape == (0, 3)
    # z-edges by (dy, dx): tt = .75 / 1, .5 / 1, (none), .5 / 1; x-edges: (dz, dy) = (1, 1) from .25 to -.5: 1 / 3;
    # y-edges: (dz, dx) = (1, 0) from -.25 to .25: 1 / 2
    pts = np.array([[1 / 3, 1, 1], [0, 0.5, 1], [0, 0, 0.75], [1, 0, 0.5], [1, 1, 0.5]])
    assert np.allclose(v[0], vol["origin"] + (0.5 + pts.mean(axis=0)) * vol["vs"], rtol=0, atol=1e-12)
    assert np.array_equal(c[0], (2 * tw["color"].reshape(8, 3).astype(int).sum(axis=0) + 8) // 16)


def test_sphere_extraction_is_a_closed_outward_surface():
    tsdf, weight, color, colored = TT.sphere_volume()
    for dtype in (np.float64, np.float32):
        v, c, f = TT.extract(tsdf, weight, color, colored, TT.SPHERE_ORIGIN, TT.SPHERE_VS, dtype=dtype)
        E, most, least = TT.mesh_topology(f)
        dist = np.abs(np.linalg.norm(v.astype(np.float64) - TT.SPHERE_CENTRE, axis=1) - TT.SPHERE_RADIUS)
        print(f"{np.dtype(dtype).name}: {v.shape[0]} vertices, {f.shape[0]} faces, {E} edges, |r - R| <= {dist.max():.3g} voxels")
        assert most == 2 and least == 2                                       # every edge belongs to exactly two faces
        assert v.shape[0] - E + f.shape[0] == 2
        assert int(f.min()) == 0 and int(f.max()) == v.shape[0] - 1           # every vertex is referenced
        p = v.astype(np.float64)
        normal = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
        assert (np.einsum("ij,ij->i", normal, p[f].mean(axis=1) - TT.SPHERE_CENTRE) > 0).all()
        assert dist.max() <= np.sqrt(3.0)                                     # the vertex lies in a cell the surface crosses
        assert (v.shape[0], f.shape[0]) == (1028, 2052)
    # a voxel without colour does not enter the mean; with none of the 8 the colour is 0
    v2, c2, f2 = TT.extract(tsdf, weight, color, np.zeros_like(colored), TT.SPHERE_ORIGIN, TT.SPHERE_VS)
    assert not c2.any() and np.array_equal(f2, f) and not np.array_equal(c, c2)
    # min_weight above every weight: nothing is valid
    v3, _, f3 = TT.extract(tsdf, weight, color, colored, TT.SPHERE_ORIGIN, TT.SPHERE_VS, min_weight=2)
    assert v3.shape[0] == 0 and f3.shape[0] == 0


def test_test_volumes_are_testable_and_exercise_every_outcome():
    for label, sc, pin in TT.shared_cases():
        tw = TT.integrate(sc, pin, TT.VOLUME)
        tw32 = TT.integrate(sc, pin, TT.VOLUME, dtype=np.float32)
        share, tol = TT.contested_share(tw), TT.tsdf_tolerance(sc, TT.VOLUME)
        free = tw["pairs"] == 0
        emu = np.abs(tw32["tsdf"].astype(np.float64) - tw["tsdf"].astype(np.float64))[free].max()
        v, _, f = TT.extract(tw["tsdf"], tw["weight"], tw["color"], tw["colored"], TT.VOLUME["origin"], TT.VOLUME["vs"])
        print(f"{label}: observed {100 * (tw['weight'] > 0).mean():.1f} %, contested {100 * share:.2f} %, tol {tol:.3g}, emulation "
              f"{emu:.3g}, {v.shape[0]} vertices, {f.shape[0]} faces")
        assert share <= TT.MAX_CONTESTED and tol <= 1e-4 and emu <= tol
        assert np.array_equal(tw32["weight"][free], tw["weight"][free])
        assert set(np.unique(tw["weight"])) == set(range(sc["K"] + 1))              # every weight 0 ... K
        assert 0 < (tw["colored"] > 0).sum() < (tw["weight"] > 0).sum()              # free space has a weight and no colour
        assert v.shape[0] > 500 and f.shape[0] > 500 and f.max() < v.shape[0]


def test_bounds_round_trip():
    for vol in (TT.VOLUME, TT.volume((10, 11, 70))):
        origin, dims = fusion.volume_grid(TT.bounds_of(vol), vol["vs"], vol["trunc"])
        assert origin.dtype == np.float32 and origin.tobytes() == vol["origin"].tobytes() and dims == vol["dims"]
    origin, dims = fusion.volume_grid(([0.01, 0.02, -0.33], [1.0, 0.5, 0.3]), 0.125, 0.25)   # padded by 0.375, snapped down
    assert origin.tolist() == [-0.375, -0.375, -0.75] and dims == (12, 10, 14)
    assert fusion.volume_grid(([0.01, 0.02, -0.33], [1.0, 0.5, 0.3]), 0.125)[1] == (16, 14, 18)   # trunc 0.5: 0.625
    assert fusion.volume_grid(([0, 0, 0], [0, 0, 0]), 1.0, 0.5)[1] == (4, 4, 4)          # a point: the padding alone


# ---- host checks -----------------------------------------------------------------------------------------------------
def frame(k, h, w, n=None):
    f = Frame(frame_id=k, img=torch.zeros(3, h, w), T_WC=torch.tensor([[0, 0, 0, 0, 0, 0, 1, 1.0]]))
    n = h * w if n is None else n
    f.X_canon, f.C, f.N = torch.ones(n, 3), torch.ones(n, 1), 1
    return f


def test_bad_arguments_raise_before_any_device_call():
    kfs, pin, box = [frame(0, 4, 5), frame(1, 4, 5)], (4.0, 4.0, 2.0, 1.5), ([0, 0, 0], [1, 1, 1])
    for kw in (dict(voxel_size=0.0), dict(voxel_size=-1.0), dict(voxel_size=float("nan")), dict(voxel_size=float("inf")),
               dict(trunc=0.0), dict(trunc=float("nan")), dict(z_min=-1e-3), dict(z_min=float("nan")),
               dict(bounds=([0, 0, 0], [1, 1])), dict(bounds=([0, 0, 0], [1, 1, float("inf")])), dict(bounds=([0, 0, 1], [1, 1, 0]))):
        with pytest.raises(ValueError):
            fusion.fuse_tsdf(kfs, pin, **{"voxel_size": 0.1, "bounds": box, **kw})
    with pytest.raises(ValueError, match="would fit") as err:
        fusion.fuse_tsdf(kfs, pin, 1e-4, bounds=box)                                     # 10^4 voxels a side
    fit = float(str(err.value).split("voxel_size of ")[1].split()[0])
    assert fusion.volume_grid(box, fit)[1] and fit < 2e-3                                # it does fit, and is not far off
    with pytest.raises(ValueError, match="4x5"):
        fusion.fuse_tsdf([frame(0, 4, 5), frame(1, 5, 4)], pin, 0.1, bounds=box)
    with pytest.raises(ValueError):
        fusion.fuse_tsdf(kfs, "guess", 0.1, bounds=box)
    with pytest.raises(ValueError):
        fusion.fuse_tsdf(kfs, (0.0, 4.0, 2.0, 1.5), 0.1, bounds=box)
    with pytest.raises(ValueError, match="bounds or out"):
        fusion.fuse_tsdf([], pin, 0.1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fusion.fuse_tsdf(kfs, pin, 0.1, bounds=box)
    vol = fusion.empty_volume([0, 0, 0], (4, 5, 6), 0.1, device="cpu")
    assert vol.dims == (4, 5, 6) and vol.trunc == float(np.float32(0.4)) and vol.color.shape == (4, 5, 6, 3)
    for kw in (dict(min_weight=0), dict(min_weight=1.5), dict(min_weight=True)):
        with pytest.raises(ValueError):
            fusion.extract_surface(vol, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fusion.extract_surface(vol)
    with pytest.raises(TypeError):
        fusion.extract_surface((vol.tsdf, vol.weight, vol.color))
    for dims in ((1, 4, 4), (4, 4, 1025), (4, 4)):
        with pytest.raises(ValueError):
            fusion.empty_volume([0, 0, 0], dims, 0.1, device="cpu")
    with pytest.raises(ValueError, match="asks for"):
        fusion.fuse_tsdf(kfs, pin, 0.2, out=vol)                                         # out's grid has another voxel size


def test_re_exports_and_signatures():
    for n in ("fuse_tsdf", "extract_surface", "TSDFVolume"):
        assert n in mast3r_utils.__all__ and n in fusion.__all__ and getattr(mast3r_utils, n) is getattr(fusion, n)
    from mast3r_slam.slam import SLAM
    E = inspect.Parameter.empty
    sig = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    assert sig(fusion.fuse_tsdf) == [("keyframes", E), ("K", E), ("voxel_size", E), ("bounds", None), ("trunc", None),
                                     ("c_conf_threshold", 1.5), ("z_min", 1e-3), ("out", None), ("workspace", None)]
    assert sig(fusion.extract_surface) == [("volume", E), ("min_weight", 1)]
    mesh = [("self", E), ("voxel_size", None), ("trunc", None), ("c_conf_threshold", 1.5), ("min_weight", 1), ("consistency", None),
            ("bounds", None)]
    assert sig(SLAM.fused_mesh) == mesh
    assert sig(SLAM.save_fused_mesh) == mesh[:1] + [("path", E)] + mesh[1:] + [("binary", True)]
    assert sig(SLAM.save_mesh) == [("self", E), ("path", E), ("c_conf_threshold", 1.5), ("stride", 1), ("edge_ratio", None),
                                   ("binary", True)]                                      # pinned: unchanged
    assert set(fusion.TSDFVolume.__dataclass_fields__) >= {"tsdf", "weight", "color", "origin", "voxel_size", "trunc"}


def test_symbols_workspaces_and_argument_validation():
    names = [n for n in _ffi.declared_symbols() if n.startswith("m3_tsdf")]
    assert sorted(names) == ["m3_tsdf_extract_count", "m3_tsdf_extract_launches", "m3_tsdf_extract_scatter", "m3_tsdf_extract_ws_bytes",
                             "m3_tsdf_integrate", "m3_tsdf_integrate_launches", "m3_tsdf_integrate_ws_bytes"]
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), n
    L = _ffi.lib()
    assert L.m3_abi_version() == 4000
    assert L.m3_tsdf_integrate_launches() == 3 and L.m3_tsdf_extract_launches() == 5
    # 64 bytes of inverse pose per keyframe, then K * N floats of planes
    assert L.m3_tsdf_integrate_ws_bytes(1, 512 * 512) == 64 + 512 * 512 * 4
    assert L.m3_tsdf_integrate_ws_bytes(64, 512 * 512) == 64 * 64 + 64 * 512 * 512 * 4 == fusion.workspace_bytes(64, 512 * 512)
    assert L.m3_tsdf_integrate_ws_bytes(0, 4) == 0 and L.m3_tsdf_integrate_ws_bytes(-1, 4) == 0 and L.m3_tsdf_integrate_ws_bytes(1, 0) == 0
    assert L.m3_tsdf_integrate_ws_bytes(1 << 11, 1 << 20) == 0                  # K * N = 2^31
    # header, two offset tables of ceil(voxels / 256) int32 (padded to 16 bytes), int32 remap and one flag byte per voxel
    pad = lambda b: (b + 15) // 16 * 16
    for dx, dy, dz in ((2, 2, 2), (45, 41, 37), (70, 3, 2), (512, 512, 512), (1024, 1024, 682)):
        total = dx * dy * dz
        blocks = (total + 255) // 256
        assert L.m3_tsdf_extract_ws_bytes(dx, dy, dz) == 16 + 2 * pad(4 * blocks) + pad(4 * total) + pad(total), (dx, dy, dz)
    for dims in ((1, 2, 2), (2, 2, 1), (1025, 2, 2), (2, 0, 2), (1024, 1024, 683), (1024, 1024, 1024)):
        assert L.m3_tsdf_extract_ws_bytes(*dims) == 0, dims                     # 3 * voxels has to stay below 2^31
    one, big = 0x1000, 1 << 40                                                  # never dereferenced: every call below is refused
    integrate = lambda **k: L.m3_tsdf_integrate(*[k.get(n, d) for n, d in (
        ("X", one), ("C", one), ("img", one), ("poses", one), ("Nk", one), ("K", 2), ("H", 4), ("W", 4), ("use", 1), ("thr", 1.5),
        ("layout", 1), ("fx", 4.0), ("fy", 4.0), ("cx", 1.5), ("cy", 1.5), ("z_min", 1e-3), ("ox", 0.0), ("oy", 0.0), ("oz", 0.0),
        ("vs", 0.1), ("trunc", 0.4), ("Dx", 8), ("Dy", 8), ("Dz", 8), ("ws", one), ("ws_bytes", big), ("tsdf", one), ("weight", one),
        ("color", one), ("colored", one), ("stream", None))])
    nan, inf = float("nan"), float("inf")
    for bad in (dict(X=None), dict(C=None), dict(img=None), dict(poses=None), dict(Nk=None), dict(ws=None), dict(tsdf=None),
                dict(weight=None), dict(color=None), dict(Dx=1), dict(Dy=1025), dict(Dz=0), dict(Dx=1024, Dy=1024, Dz=1024 + 1),
                dict(ox=nan), dict(oy=inf), dict(oz=-inf), dict(vs=0.0), dict(vs=nan), dict(vs=inf), dict(vs=-0.1), dict(trunc=0.0),
                dict(trunc=nan), dict(trunc=inf), dict(z_min=-1.0), dict(z_min=nan), dict(use=2), dict(layout=2), dict(H=0),
                dict(H=1 << 16, W=1 << 16), dict(fx=0.0), dict(fy=inf), dict(cx=nan), dict(ws_bytes=64), dict(ws=one + 4),
                dict(tsdf=one + 2), dict(weight=one + 1), dict(K=-1)):
        assert integrate(**bad) == -1, bad
    count = lambda **k: L.m3_tsdf_extract_count(*[k.get(n, d) for n, d in (
        ("tsdf", one), ("weight", one), ("Dx", 8), ("Dy", 8), ("Dz", 8), ("min_weight", 1), ("ws", one), ("ws_bytes", big),
        ("stream", None))])
    for bad in (dict(tsdf=None), dict(weight=None), dict(ws=None), dict(Dx=1), dict(Dz=1025), dict(Dx=1024, Dy=1024, Dz=1024),
                dict(min_weight=0), dict(ws=one + 8), dict(ws_bytes=16), dict(tsdf=one + 1)):
        assert count(**bad) == -1, bad
    scatter = lambda **k: L.m3_tsdf_extract_scatter(*[k.get(n, d) for n, d in (
        ("tsdf", one), ("weight", one), ("color", one), ("colored", one), ("ox", 0.0), ("oy", 0.0), ("oz", 0.0), ("vs", 0.1), ("Dx", 8),
        ("Dy", 8), ("Dz", 8), ("min_weight", 1), ("ws", one), ("ws_bytes", big), ("V", 4), ("F", 4), ("vertices", one), ("colors", one),
        ("faces", one), ("stream", None))])
    for bad in (dict(tsdf=None), dict(weight=None), dict(color=None), dict(ws=None), dict(vertices=None), dict(colors=None),
                dict(faces=None), dict(Dy=1), dict(ox=nan), dict(vs=0.0), dict(vs=inf), dict(min_weight=0), dict(V=0), dict(F=0),
                dict(F=3), dict(V=513), dict(F=6 * 512 + 2), dict(ws=one + 4), dict(ws_bytes=16), dict(vertices=one + 2),
                dict(faces=one + 1)):
        assert scatter(**bad) == -1, bad
