"""CPU: the renderer's float64 twin (tests/render_twin.py) on hand-made scenes with known answers, the scenes the GPU
tests use (exact scenes are exact in fp32; general scenes stay under the contested-pixel cap), the closed forms of the
camera helpers, argument errors and the exported symbols."""
import math

import numpy as np
import pytest
import torch

import render_scenes as RS
import render_twin as RT
from mast3r_slam import _ffi, mast3r_utils, render
from mast3r_slam.frame import Frame, Keyframes

IDENT = np.array([0, 0, 0, 0, 0, 0, 1, 1], dtype=np.float32)
KCAM = (4.0, 4.0, 2.0, 1.0)                                               # pixel (x, y) sees the ray ((x - 2) / 4, (y - 1) / 4, 1)
SIZE = (3, 5)


def scene(points, conf=None, colours=None):
    X = np.asarray(points, dtype=np.float32)[None]
    N = X.shape[1]
    C = np.full((1, N), 2.0, dtype=np.float32) if conf is None else np.asarray(conf, dtype=np.float32)[None]
    img = (np.arange(3 * N, dtype=np.uint8).reshape(1, N, 3) + 10) if colours is None else np.asarray(colours, dtype=np.uint8)[None]
    return dict(X=X, C=C, Nk=np.array([1], dtype=np.int32), T=IDENT[None].copy(), img=img, layout="u8", K=1, N=N)


def at(x, y, z):
    return [z * (x - 2) / 4, z * (y - 1) / 4, z]


def test_one_point_per_pixel():
    pts = [at(x, y, 2.0 + 0.25 * (y * 5 + x)) for y in range(3) for x in range(5)]
    tw = RT.render_twin(scene(pts), IDENT, KCAM, SIZE)
    assert np.array_equal(tw["index"], np.arange(15).reshape(3, 5))
    assert np.array_equal(tw["depth"], 2.0 + 0.25 * np.arange(15).reshape(3, 5))
    assert np.array_equal(tw["rgb"].reshape(15, 3), np.arange(45, dtype=np.uint8).reshape(15, 3) + 10)


def test_nearer_wins_and_equal_depth_goes_to_the_smaller_index():
    tw = RT.render_twin(scene([at(1, 1, 4.0), at(1, 1, 2.0), at(3, 2, 2.0), at(3, 2, 2.0)]), IDENT, KCAM, SIZE)
    assert tw["index"][1, 1] == 1 and tw["depth"][1, 1] == 2.0
    assert tw["index"][2, 3] == 2
    assert int((tw["index"] >= 0).sum()) == 2 and np.isposinf(tw["depth"][0, 0])
    assert tw["contested"][2, 3] and tw["contested"][1, 1] == False         # a tie in depth is contested, a clear win is not


def test_rejected_sources_leave_the_background():
    pts = [at(1, 1, -2.0), at(2, 1, 50.0), at(7, 1, 2.0), at(2, -3, 2.0), [np.nan, 0, 2.0], at(3, 1, 2.0), at(0, 0, 2.0)]
    conf = [2, 2, 2, 2, 2, 1.5, 2]                                          # the sixth sits exactly at the threshold: strict
    tw = RT.render_twin(scene(pts, conf), IDENT, KCAM, SIZE, far=40.0, background=(1, 2, 3))
    assert int((tw["index"] >= 0).sum()) == 1 and tw["index"][0, 0] == 6
    assert (tw["rgb"][1, 1] == (1, 2, 3)).all() and np.isposinf(tw["depth"][1, 3])
    tw = RT.render_twin(scene(pts, conf), IDENT, KCAM, SIZE, far=40.0, thr=None)
    assert tw["index"][1, 3] == 5                                           # without the threshold it is drawn
    assert RT.render_twin(scene(pts, conf), IDENT, KCAM, SIZE, thr=np.inf)["covered"].sum() == 0


def test_footprint_and_pixel_centres():
    tw = RT.render_twin(scene([at(0, 0, 2.0), at(2.49, 1.49, 3.0), at(2.51, 1, 4.0)]), IDENT, KCAM, SIZE, point_size=3)
    want = np.full((3, 5), -1)
    want[0:2, 0:2] = 0                                                      # clipped at the corner
    want[0:3, 1:4] = np.where(want[0:3, 1:4] == 0, 0, 1)                    # (2.49, 1.49) rounds to pixel (2, 1)
    want[0:3, 4] = 2                                                        # (2.51, 1) rounds to pixel (3, 1); nearer points win 2..3
    assert np.array_equal(tw["index"], want)


def test_view_pose_is_inverted():
    view = np.array([1, 2, 3, 0.5, 0.5, 0.5, 0.5, 2], dtype=np.float32)     # a third turn: x -> y -> z -> x, scale 2
    c = np.array(at(3, 2, 4.0))
    p = 2.0 * (RS.rot(view[3:7].astype(np.float64)) @ c) + view[:3]
    tw = RT.render_twin(scene([p]), view, KCAM, SIZE)
    assert tw["index"][2, 3] == 0 and tw["depth"][2, 3] == 4.0


@pytest.mark.parametrize("layout", ["f32", "u8"])
@pytest.mark.parametrize("K,N", [(1, 4999), (3, 4097), (17, 1023)])
def test_exact_scenes_are_exact_in_fp32(K, N, layout):
    """The promise of render_scenes.exact_scene: the rule evaluated in float32 equals the rule in float64, bit for bit."""
    for ps, far in ((1, np.inf), (5, 4.0)):
        sc, view, Kc = RS.exact_scene(K, N, seed=K + N, layout=layout)
        tw = RT.render_twin(sc, view, Kc, (61, 83), near=0.125, far=far, point_size=ps)
        rgb, depth, index = RT.fp32_emulation(sc, view, Kc, (61, 83), near=0.125, far=far, point_size=ps)
        assert np.array_equal(index, tw["index"]) and np.array_equal(rgb, tw["rgb"])
        assert np.array_equal(depth.astype(np.float64), tw["depth"])
        assert tw["covered"].mean() > 0.1                                      # the scene draws something
    cand, u, v, z, _ = RT.sources(sc, view, Kc, 0.125, np.inf, 1.5)
    px = np.floor(u + 0.5)[cand & (z > 0)]
    assert np.unique(np.stack([px, np.floor(v + 0.5)[cand & (z > 0)], z[cand & (z > 0)]]), axis=1).shape[1] < px.size   # ties exist


GENERAL = [(1, 1, 4999, 240, 320), (3, 1, 4999, 240, 320), (1, 128, 256, 240, 320), (3, 128, 256, 240, 320)]


@pytest.mark.parametrize("where", ["inside", "back"])
@pytest.mark.parametrize("K,H,W,Hv,Wv", GENERAL)
def test_general_scenes_stay_under_the_contested_cap(K, H, W, Hv, Wv, where):
    """The scenes of tests/test_gpu_render.py, twin alone: contested share under the cap, and the float32 emulation of the
    rule passes the device's check."""
    sc = RS.general_scene(K, H, W, seed=K + W, layout="u8")
    view, Kc = RS.general_view((Hv, Wv), where)
    for thr in (None, 1.5):
        tw = RT.render_twin(sc, view, Kc, (Hv, Wv), near=0.5, thr=thr)
        rgb, depth, index = RT.fp32_emulation(sc, view, Kc, (Hv, Wv), near=0.5, thr=thr)
        share = RT.check_against_twin(tw, rgb, depth, index, f"K={K} {H}x{W} -> {Hv}x{Wv} {where} thr={thr}")
        per_pixel = float((tw["src"]["ok"]).sum()) / max(1, int(tw["covered"].sum()))
        print(f"  {per_pixel:.2f} sources per covered pixel")
        assert share <= RT.MAX_CONTESTED and tw["covered"].sum() > 1000


def test_default_intrinsics_look_at_and_behind():
    fx, fy, cx, cy = render.default_intrinsics((480, 640), 90.0)
    assert fx == pytest.approx(320.0) and fy == fx and (cx, cy) == (319.5, 239.5)
    assert render.default_intrinsics((480, 640))[0] == pytest.approx(320.0 / math.tan(math.radians(30.0)))
    with pytest.raises(ValueError):
        render.default_intrinsics((0, 640))
    T = render.look_at((1, 2, 3), (1, 2, 10))                                # looking along +z with y down: the identity
    assert T.shape == (1, 8) and T.dtype == torch.float32
    assert np.allclose(T.numpy()[0], [1, 2, 3, 0, 0, 0, 1, 1], atol=1e-7)
    T = render.look_at((0, 0, 0), (5, 0, 0)).numpy()[0].astype(np.float64)   # looking along +x: z -> x, y stays down
    R = RS.rot(T[3:7])
    assert np.allclose(R @ [0, 0, 1], [1, 0, 0], atol=1e-6) and np.allclose(R @ [0, 1, 0], [0, 1, 0], atol=1e-6)
    assert np.allclose(R @ [1, 0, 0], [0, 0, -1], atol=1e-6) and np.linalg.det(R) == pytest.approx(1.0)
    for eye, target in (((3, -1, 2), (0, 0.5, -4)), ((0, 0, 0), (-1, 0.2, -1)), ((1, 1, 1), (1, 1.5, 0))):
        T = render.look_at(eye, target).numpy()[0].astype(np.float64)
        R = RS.rot(T[3:7])
        fwd = np.subtract(target, eye) / np.linalg.norm(np.subtract(target, eye))
        assert np.allclose(R @ [0, 0, 1], fwd, atol=1e-6) and np.allclose(R.T @ R, np.eye(3), atol=1e-6)
        assert (R @ [0, 1, 0])[1] > 0 and abs((R @ [1, 0, 0])[1]) < 1e-6     # y keeps pointing down, x stays horizontal
        assert T[6] >= 0 and T[7] == 1
    with pytest.raises(ValueError):
        render.look_at((0, 0, 0), (0, 0, 0))
    with pytest.raises(ValueError):
        render.look_at((0, 0, 0), (0, 3, 0))
    pose = torch.tensor([[1.0, 2.0, 3.0, 0.5, 0.5, 0.5, 0.5, 1.7]])          # x -> y -> z -> x
    B = render.behind(pose, distance=2.0, height=0.5).numpy()[0]
    assert np.allclose(B, [1 - 2.0, 2.0, 3 - 0.5, 0.5, 0.5, 0.5, 0.5, 1.0], atol=1e-6)   # back along R e_z = e_x, up along -R e_y = -e_z
    assert np.allclose(render.behind(pose, 0.0, 0.0).numpy()[0, :7], pose.numpy()[0, :7])
    assert render.scaled_intrinsics((100.0, 100.0, 49.5, 24.5), (50, 100), (100, 200)) == (200.0, 200.0, 99.5, 49.5)


def frame(i, n, img, count=1):
    f = Frame(frame_id=i, img=img, T_WC=torch.tensor([[0, 0, 0, 0, 0, 0, 1, 1.0]]))
    f.X_canon, f.C, f.N = torch.zeros(n, 3), torch.ones(n, 1), count
    return f


def test_render_map_argument_errors():
    ok, pose = torch.zeros(3, 4, 5), torch.tensor([[0, 0, 0, 0, 0, 0, 1, 1.0]])
    K, size = (10.0, 10.0, 2.0, 2.0), (4, 5)
    for ps in (0, 2, 9, -1):
        with pytest.raises(ValueError, match="point_size"):
            render.render_map([frame(0, 20, ok)], pose, K, size, point_size=ps)
    for bad in ((0.0, 10.0, 2, 2), (10.0, -1.0, 2, 2), (10.0, math.inf, 2, 2), (1, 2, 3)):
        with pytest.raises(ValueError):
            render.render_map([frame(0, 20, ok)], pose, bad, size)
    for bad in ((0, 5), (4, -1), (4,), (4, 20000)):
        with pytest.raises(ValueError):
            render.render_map([frame(0, 20, ok)], pose, K, bad)
    for near, far in ((1.0, 1.0), (2.0, 1.0), (-1.0, 1.0), (math.nan, 1.0)):
        with pytest.raises(ValueError, match="near"):
            render.render_map([frame(0, 20, ok)], pose, K, size, near=near, far=far)
    with pytest.raises(ValueError, match="background"):
        render.render_map([frame(0, 20, ok)], pose, K, size, background=(0, 0, 256))
    with pytest.raises(ValueError, match="points"):
        render.render_map([frame(0, 20, ok), frame(1, 24, torch.zeros(3, 4, 6))], pose, K, size)
    with pytest.raises(ValueError, match="mix"):
        render.render_map([frame(0, 20, ok), frame(1, 20, torch.zeros(4, 5, 3, dtype=torch.uint8))], pose, K, size)
    with pytest.raises(ValueError, match="image"):
        render.render_map([frame(0, 20, torch.zeros(20, 3))], pose, K, size)
    with pytest.raises(RuntimeError):                                         # valid, but on the CPU
        render.render_map([frame(0, 20, ok)], pose, K, size)
    with pytest.raises(RuntimeError):                                         # an empty map still needs a device pose
        render.render_map(Keyframes(), pose, K, size)
    with pytest.raises(ValueError):
        render.ViewRecorder(".", every=0)
    with pytest.raises(ValueError):
        render.ViewRecorder(".", camera="orbit")
    with pytest.raises(ValueError):
        render.save_image("x.png", np.zeros((4, 5), dtype=np.uint8))


def test_depth_to_rgb_and_save_image(tmp_path):
    d = torch.tensor([[1.0, 2.0, 3.0], [math.inf, 1.5, 3.0]])
    g = render.depth_to_rgb(d)
    assert g.shape == (2, 3, 3) and g.dtype == torch.uint8
    assert g[0, 0].tolist() == [255] * 3 and g[0, 2].tolist() == [32] * 3 and g[1, 0].tolist() == [0] * 3
    assert g[0, 0, 0] > g[1, 1, 0] > g[0, 1, 0] > g[0, 2, 0]
    assert render.depth_to_rgb(d, near=0.0, far=6.0)[0, 2].tolist() == [143] * 3       # 255 - 223 * 0.5, floored
    from PIL import Image
    rgb = torch.arange(2 * 3 * 3, dtype=torch.uint8).reshape(2, 3, 3)
    render.save_image(tmp_path / "v.png", rgb)
    back = np.asarray(Image.open(tmp_path / "v.png"))
    assert back.shape == (2, 3, 3) and np.array_equal(back, rgb.numpy())


def test_symbols_are_declared_exported_and_validate():
    names = _ffi.declared_symbols()
    for n in ("m3_render_ws_bytes", "m3_render_launches", "m3_render_map"):
        assert n in names
    for n in render.__all__:
        assert n in mast3r_utils.__all__ and getattr(mast3r_utils, n) is getattr(render, n)
    L = _ffi.lib()
    assert L.m3_abi_version() == 4000                                         # symbols were added, nothing changed
    assert L.m3_render_ws_bytes(480, 640) == 480 * 640 * 8 and L.m3_render_ws_bytes(1, 1) == 8
    assert L.m3_render_ws_bytes(0, 640) == 0 and L.m3_render_ws_bytes(480, 16385) == 0
    assert L.m3_render_launches(1) == 3 and L.m3_render_launches(256) == 3 and L.m3_render_launches(0) == 2
    args = [None, None, None, None, None, 1, 4, 1, 1.5, 0, None, 10.0, 10.0, 2.0, 2.0, 4, 5, 0.1, 10.0, 1, 0, 0, 0, None, 160,
            None, None, None, None]
    assert L.m3_render_map(*args) == -1                                       # NULL pointers: refused before any launch
