"""CPU: the mesh rule as tests/mesh_twin.py restates it (analytic plane and step, scenes that are not vacuous), the PLY
mesh writer, the argument checks of collect_mesh and the entry points' validation."""
import inspect

import numpy as np
import pytest
import torch

import mesh_twin as MT
from mast3r_slam import _ffi, export, mast3r_utils
from mast3r_slam.frame import Frame

PLY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
HEADER = ["property float x", "property float y", "property float z", "property uchar red", "property uchar green",
          "property uchar blue"]


# ---- 1. the scenes of the GPU tests are not vacuous --------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in MT.CASES])
def test_scenes_keep_between_20_and_80_percent_of_the_candidates(name):
    sc, thr, stride, ratio = MT.case_scene(name)
    faces, used, cand = MT.mesh_twin(sc, thr, stride, ratio)
    print(f"{name}: {faces.shape[0]} of {cand} candidate faces kept, {used.size} vertices")
    assert cand == 2 * sc["K"] * (-(-sc["H"] // stride) - 1) * (-(-sc["W"] // stride) - 1)
    assert 0.2 * cand <= faces.shape[0] <= 0.8 * cand
    per_kf = np.bincount(faces[:, 0] // (sc["H"] * sc["W"]), minlength=sc["K"])
    if name in ("33x65", "33x65 stride 2", "33x65 stride 3"):
        assert per_kf[0] > 0 and per_kf[1] == 0 and per_kf[2] > 0            # an empty keyframe between two that keep faces
    else:
        assert (per_kf > 0).all()


def test_the_small_scenes_keep_what_their_docstrings_say():
    faces, used, cand = MT.mesh_twin(MT.one_cell_scene("u8"), MT.THR, 1, 0.8)
    assert cand == 2 and faces.tolist() == [[0, 2, 1]] and used.tolist() == [0, 1, 2]
    faces, used, cand = MT.mesh_twin(MT.bound_scene(), MT.THR, 1, 0.5)
    assert cand == 4 and faces.tolist() == [[0, 2, 1]]                        # on the bound: kept; an ulp past it: dropped
    assert MT.mesh_twin(MT.make_scene(1, 1, 8, 0, "u8"), None, 1, 1.0)[2] == 0
    assert MT.mesh_twin(MT.make_scene(1, 8, 1, 0, "u8"), None, 1, 1.0)[2] == 0


# ---- 2. analytic plane and step ------------------------------------------------------------------------------------
def flat_scene(K, H, W, depth):
    """A pinhole with f = W looking at depth(u) (a function of the column), everything confident, random poses."""
    sc = MT.make_scene(K, H, W, seed=3, layout="u8", pitch=H + W, block=(0, 0))
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.stack([(u - (W - 1) / 2) / W, (v - (H - 1) / 2) / W, np.ones_like(u)], axis=-1)
    sc["X"][:] = (depth(u)[..., None] * ray).reshape(H * W, 3).astype(np.float32)
    sc["C"][:] = 2.0 * sc["Nk"][:, None]
    return sc


@pytest.mark.parametrize("stride", [1, 2, 3])
def test_a_plane_keeps_every_face_and_faces_look_at_the_camera(stride):
    K, H, W = 2, 11, 13                                                       # neither is a multiple of 2 or 3
    sc = flat_scene(K, H, W, lambda u: 2.0 + 0.0 * u)
    faces, used, cand = MT.mesh_twin(sc, MT.THR, stride, 0.2 * stride)        # a pixel step is about 1 / 13 of the range
    Hg, Wg = -(-H // stride), -(-W // stride)
    assert faces.shape[0] == cand == 2 * K * (Hg - 1) * (Wg - 1)
    assert used.size == K * Hg * Wg
    P = sc["X"].reshape(K * H * W, 3).astype(np.float64)[faces]               # camera-frame corners [F,3,3]
    normal = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    assert ((normal * P.mean(axis=1)).sum(axis=1) < 0).all()


@pytest.mark.parametrize("stride", [1, 2, 3])
def test_a_step_is_not_bridged(stride):
    K, H, W, edge = 2, 11, 13, 7                                              # columns >= 7 are near, the others far
    sc = flat_scene(K, H, W, lambda u: np.where(u >= edge, 1.0, 2.0))
    faces, used, cand = MT.mesh_twin(sc, MT.THR, stride, 0.2 * stride)
    near = (faces % W) >= edge
    assert (near.all(axis=1) | (~near).all(axis=1)).all()
    Hg = -(-H // stride)
    assert faces.shape[0] == cand - 2 * K * (Hg - 1)                          # one column of cells touches the step
    assert 0 < edge % stride or stride == 1                                   # ... and the step is between two grid columns


# ---- 3. the PLY writer -----------------------------------------------------------------------------------------------
def read_ply_mesh(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines()
    v, f = int(lines[2].split()[-1]), int(lines[9].split()[-1])
    assert lines[0] == "ply" and lines[2] == f"element vertex {v}" and lines[3:9] == HEADER
    assert lines[9:] == [f"element face {f}", "property list uchar int vertex_indices", "end_header"]
    if lines[1] == "format binary_little_endian 1.0":
        assert len(raw) == end + 15 * v + 13 * f
        body = np.frombuffer(raw, dtype=PLY_DTYPE, count=v, offset=end)
        tri = np.frombuffer(raw, dtype=FACE_DTYPE, count=f, offset=end + 15 * v)
        assert (tri["n"] == 3).all()
        return (np.stack([body["x"], body["y"], body["z"]], axis=1).reshape(v, 3),
                np.stack([body["red"], body["green"], body["blue"]], axis=1).reshape(v, 3), tri["v"].reshape(f, 3))
    assert lines[1] == "format ascii 1.0"
    rows = [r.split() for r in raw[end:].decode("ascii").splitlines()]
    assert len(rows) == v + f and all(r[0] == "3" and len(r) == 4 for r in rows[v:])
    return (np.array([r[:3] for r in rows[:v]], dtype=np.float64).reshape(v, 3),
            np.array([r[3:] for r in rows[:v]], dtype=np.int64).reshape(v, 3),
            np.array([r[1:] for r in rows[v:]], dtype=np.int64).reshape(f, 3))


def small_mesh(v, f, seed=0):
    rng = np.random.default_rng(seed)
    p = (rng.normal(size=(v, 3)) * 10).astype(np.float32)
    c = rng.integers(0, 256, size=(v, 3)).astype(np.uint8)
    t = rng.integers(0, max(v, 1), size=(f, 3)).astype(np.int32)
    return p, c, t


@pytest.mark.parametrize("v,f", [(0, 0), (3, 1), (500, 900)])
@pytest.mark.parametrize("as_tensor", [False, True])
def test_save_ply_mesh_round_trip(tmp_path, v, f, as_tensor):
    p, c, t = small_mesh(v, f)
    args = [torch.from_numpy(a) for a in (p, c, t)] if as_tensor else [p, c, t]
    assert export.save_ply_mesh(tmp_path / "m.ply", *args) == (v, f)
    pb, cb, tb = read_ply_mesh(tmp_path / "m.ply")
    assert pb.tobytes() == p.tobytes() and np.array_equal(cb, c) and np.array_equal(tb, t) and tb.dtype == np.int32
    assert export.save_ply_mesh(tmp_path / "a.ply", *args, binary=False) == (v, f)
    pa, ca, ta = read_ply_mesh(tmp_path / "a.ply")
    assert np.array_equal(ca, c) and np.array_equal(ta, t)
    assert np.abs(pa - p).max(initial=0.0) <= 0.5e-6 + 1e-12                  # %.6f


def test_save_ply_mesh_rejects_bad_input(tmp_path):
    p, c, t = small_mesh(5, 4)
    for bad in (5, -1):
        t2 = t.copy()
        t2[2, 1] = bad
        with pytest.raises(ValueError, match="face"):
            export.save_ply_mesh(tmp_path / "x.ply", p, c, t2)
    with pytest.raises(ValueError):
        export.save_ply_mesh(tmp_path / "x.ply", p, c[:4], t)
    with pytest.raises(ValueError, match="face"):
        export.save_ply_mesh(tmp_path / "x.ply", p[:0], c[:0], t)             # faces without vertices


# ---- 4. collect_mesh argument checks, re-exports, signatures -------------------------------------------------------------
def frame(i, h, w):
    f = Frame(frame_id=i, img=torch.zeros(3, h, w), T_WC=torch.tensor([[0, 0, 0, 0, 0, 0, 1, 1.0]]))
    f.X_canon, f.C, f.N = torch.zeros(h * w, 3), torch.ones(h * w, 1), 1
    return f


def test_collect_mesh_argument_errors():
    with pytest.raises(RuntimeError):                                          # valid, but on the CPU: there is no CPU path
        export.collect_mesh([frame(0, 4, 5)])
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError, match="stride"):
            export.collect_mesh([frame(0, 4, 5)], stride=bad)
    for bad in (0.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="edge_ratio"):
            export.collect_mesh([frame(0, 4, 5)], edge_ratio=bad)
    with pytest.raises(ValueError, match="4x5"):
        export.collect_mesh([frame(0, 4, 5), frame(1, 5, 4)])                  # the same point count, another grid


def test_collect_mesh_without_keyframes_is_empty():
    empty = Frame(frame_id=0, img=torch.zeros(3, 4, 5), T_WC=torch.zeros(1, 8))   # no pointmap: skipped
    for kfs in ([], [empty]):
        v, c, f, i = export.collect_mesh(kfs, return_index=True)
        assert v.shape == (0, 3) and v.dtype == torch.float32 and c.shape == (0, 3) and c.dtype == torch.uint8
        assert f.shape == (0, 3) and f.dtype == torch.int32 and i.shape == (0,) and i.dtype == torch.int64
        assert len(export.collect_mesh(kfs)) == 3


def test_re_exports_and_signatures():
    for n in ("collect_mesh", "save_ply_mesh"):
        assert n in mast3r_utils.__all__ and n in export.__all__ and getattr(mast3r_utils, n) is getattr(export, n)
    from mast3r_slam.slam import SLAM
    E = inspect.Parameter.empty
    sig = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    assert sig(export.collect_mesh) == [("keyframes", E), ("c_conf_threshold", 1.5), ("stride", 1), ("edge_ratio", None),
                                        ("return_index", False)]
    assert sig(export.save_ply_mesh) == [("path", E), ("vertices", E), ("colors", E), ("faces", E), ("binary", True)]
    assert sig(SLAM.save_mesh) == [("self", E), ("path", E), ("c_conf_threshold", 1.5), ("stride", 1), ("edge_ratio", None),
                                   ("binary", True)]
    assert sig(SLAM.mesh)[:4] == [("self", E), ("c_conf_threshold", 1.5), ("stride", 1), ("edge_ratio", None)]


def test_entry_points_validate_before_any_device_call():
    names = _ffi.declared_symbols()
    for n in ("m3_mesh_ws_bytes", "m3_mesh_launches", "m3_mesh_count", "m3_mesh_scatter"):
        assert n in names
    L = _ffi.lib()
    assert L.m3_mesh_launches() == 5
    # header 16, 256 vertex tiles of 1024 points, 511 * 2 face segments of 256 cells (padded to 1024), remap, a byte per cell
    assert L.m3_mesh_ws_bytes(1, 512, 512, 1) == 16 + 256 * 4 + 1024 * 4 + 512 * 512 * 4 + (511 * 511 + 15) // 16 * 16
    assert L.m3_mesh_ws_bytes(0, 4, 4, 1) == 16 and L.m3_mesh_ws_bytes(3, 1, 8, 1) == 16 == L.m3_mesh_ws_bytes(3, 8, 4, 4)
    assert L.m3_mesh_ws_bytes(1, 4, 4, 0) == 0 and L.m3_mesh_ws_bytes(1, 0, 4, 1) == 0 and L.m3_mesh_ws_bytes(-1, 4, 4, 1) == 0
    assert L.m3_mesh_ws_bytes(1, 1 << 16, 1 << 16, 1) == 0                    # H * W overflows
    assert L.m3_mesh_ws_bytes(1 << 11, 1 << 10, 1 << 10, 1) == 0              # K * H * W = 2^31
    assert L.m3_mesh_ws_bytes(1 << 11, 1 << 10, 1 << 10, 2) == 0              # the points decide, whatever the stride
    assert L.m3_mesh_ws_bytes(1024, 1025, 1025, 1) == 0                       # 2 * cells = 2 * 1024^3 = 2^31
    assert L.m3_mesh_ws_bytes(1024, 1025, 1025, 2) > 0 and L.m3_mesh_ws_bytes(1023, 1025, 1025, 1) > 0
    one, big = 0x1000, 1 << 30                                                # never dereferenced: every call below is refused
    count = lambda **k: L.m3_mesh_count(*[k.get(n, d) for n, d in (
        ("X", one), ("C", one), ("poses", one), ("Nk", one), ("K", 1), ("H", 4), ("W", 4), ("stride", 1), ("use", 1),
        ("thr", 1.5), ("ratio", 0.1), ("ws", one), ("ws_bytes", big), ("stream", None))])
    for bad in (dict(ws=None), dict(stride=0), dict(ratio=0.0), dict(ratio=-1.0), dict(ratio=float("nan")), dict(ws_bytes=64),
                dict(H=1 << 16, W=1 << 16), dict(X=None), dict(C=None), dict(poses=None), dict(Nk=None), dict(use=2),
                dict(ws=one + 4)):
        assert count(**bad) == -1, bad
    scatter = lambda **k: L.m3_mesh_scatter(*[k.get(n, d) for n, d in (
        ("X", one), ("C", one), ("img", one), ("poses", one), ("Nk", one), ("K", 1), ("H", 4), ("W", 4), ("stride", 1),
        ("use", 1), ("thr", 1.5), ("ratio", 0.1), ("layout", 0), ("ws", one), ("ws_bytes", big), ("V", 4), ("F", 2),
        ("vertices", one), ("colors", one), ("faces", one), ("index", None), ("stream", None))])
    for bad in (dict(ws=None), dict(stride=0), dict(ratio=float("nan")), dict(ws_bytes=64), dict(img=None), dict(V=0), dict(F=0),
                dict(V=17), dict(F=19), dict(layout=2), dict(vertices=None), dict(colors=None), dict(faces=None), dict(K=0),
                dict(H=1)):
        assert scatter(**bad) == -1, bad
