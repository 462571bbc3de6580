"""GPU: the headless renderer (csrc/render.hip through render.render_map) against its float64 twin (tests/render_twin.py).

Exact scenes (tests/render_scenes.exact_scene: every fp32 operation of the rule is exact) must match the twin byte for
byte.  General scenes must match it on every uncontested pixel (index and colour exactly, depth within a relative 1e-5)
and give -1 or a listed candidate on a contested one; a scene whose contested pixels exceed 5 % of its covered pixels
fails as untestable.  The footprint, the agreement with the exporter, determinism and graph capture are exact."""
import numpy as np
import pytest
import torch

import render_scenes as RS
import render_twin as RT
from mast3r_slam import _ffi, export, render

pytestmark = pytest.mark.gpu
NEAR = 0.5


def draw(frames, view, Kc, size, dev, **kw):
    view_t = view if isinstance(view, torch.Tensor) else torch.from_numpy(np.asarray(view, dtype=np.float32)).to(dev)
    rgb, depth, index = render.render_map(frames, view_t, Kc, size, return_index=True, **kw)
    assert rgb.dtype == torch.uint8 and depth.dtype == torch.float32 and index.dtype == torch.int64
    return rgb.cpu().numpy(), depth.cpu().numpy(), index.cpu().numpy()


# ---- 1. exact scenes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["f32", "u8"])
@pytest.mark.parametrize("K,N", [(1, 4999), (3, 4097), (17, 1023), (3, 4096)])
def test_exact_scenes_are_byte_equal(dev, K, N, layout):
    size = (61, 83) if N % 4 else (64, 80)                                  # 5063 pixels: the scalar tail of clear and resolve
    sc, view, Kc = RS.exact_scene(K, N, seed=K + N, layout=layout, size=size)
    frames = RS.frames_of(sc, dev)
    for ps, far, thr, bg in ((1, np.inf, 1.5, (0, 0, 0)), (5, 4.0, 1.5, (7, 8, 9)), (1, np.inf, None, (255, 0, 1))):
        tw = RT.render_twin(sc, view, Kc, size, near=0.125, far=far, thr=thr, point_size=ps, background=bg)
        rgb, depth, index = draw(frames, view, Kc, size, dev, near=0.125, far=far, c_conf_threshold=thr, point_size=ps,
                                 background=bg)
        ties = int((tw["contested"] & tw["covered"]).sum())
        print(f"K={K} N={N} {layout} ps={ps} far={far} thr={thr}: covered {int(tw['covered'].sum())} of {size[0] * size[1]}, "
              f"{ties} pixels with a tie or an exact half-pixel source")
        assert ties > 0
        assert np.array_equal(index, tw["index"])
        assert np.array_equal(rgb, tw["rgb"])
        assert depth.tobytes() == tw["depth"].astype(np.float32).tobytes()


def test_unaligned_inputs_and_outputs_take_the_scalar_path(dev):
    sc, view, Kc = RS.exact_scene(3, 4096, seed=9, layout="f32", size=(64, 80))
    frames = RS.frames_of(sc, dev)
    ref = draw(frames, view, Kc, (64, 80), dev, near=0.125, point_size=3)
    for f in frames:
        for name in ("X_canon", "C", "img"):
            t = getattr(f, name)
            buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
            buf[1:] = t.reshape(-1)
            setattr(f, name, buf[1:].view(t.shape))
            assert getattr(f, name).data_ptr() % 16 != 0
    P = 64 * 80
    out = (torch.empty(3 * P + 1, dtype=torch.uint8, device=dev)[1:].view(64, 80, 3),
           torch.empty(P + 1, dtype=torch.float32, device=dev)[1:].view(64, 80),
           torch.empty(P + 1, dtype=torch.int64, device=dev)[1:].view(64, 80))
    assert out[0].data_ptr() % 4 and out[1].data_ptr() % 16 and out[2].data_ptr() % 16
    got = draw(frames, view, Kc, (64, 80), dev, near=0.125, point_size=3, out=out)
    for a, b in zip(ref, got):
        assert a.tobytes() == b.tobytes()
    tw = RT.render_twin(sc, view, Kc, (64, 80), near=0.125, point_size=3)
    assert np.array_equal(got[2], tw["index"]) and np.array_equal(got[0], tw["rgb"])


# ---- 2. general scenes ---------------------------------------------------------------------------------------------
GENERAL = [(1, 1, 4999, 240, 320), (3, 1, 4999, 240, 320), (1, 128, 256, 240, 320), (3, 128, 256, 240, 320),
           (1, 512, 512, 1080, 1920), (3, 512, 512, 1080, 1920)]


@pytest.mark.parametrize("layout", ["f32", "u8"])
@pytest.mark.parametrize("where", ["inside", "back"])
@pytest.mark.parametrize("K,H,W,Hv,Wv", GENERAL)
def test_general_scenes_against_the_twin(dev, K, H, W, Hv, Wv, where, layout):
    sc = RS.general_scene(K, H, W, seed=K + W, layout=layout)
    view, Kc = RS.general_view((Hv, Wv), where)
    frames = RS.frames_of(sc, dev)
    for thr in (None, 1.5):
        tw = RT.render_twin(sc, view, Kc, (Hv, Wv), near=NEAR, thr=thr)
        rgb, depth, index = draw(frames, view, Kc, (Hv, Wv), dev, near=NEAR, c_conf_threshold=thr)
        RT.check_against_twin(tw, rgb, depth, index, f"K={K} {H}x{W} -> {Hv}x{Wv} {where} {layout} thr={thr}")
        assert tw["covered"].sum() > 1000
    rgb, depth, index = draw(frames, view, Kc, (Hv, Wv), dev, near=NEAR, c_conf_threshold=float("inf"), background=(3, 2, 1))
    assert (index == -1).all() and np.isposinf(depth).all() and (rgb == (3, 2, 1)).all()


# ---- 3. footprint ----------------------------------------------------------------------------------------------------
def keys_of(depth, index):
    return np.where(index >= 0, (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (index.astype(np.uint64) & np.uint64(0xffffffff)),
                    np.uint64(0xffffffffffffffff))


@pytest.mark.parametrize("ps", [3, 5, 7])
def test_footprint_is_the_window_minimum_of_point_size_one(dev, ps):
    sc = RS.general_scene(3, 128, 256, seed=4, layout="u8")
    view, Kc = RS.general_view((240, 320), "inside")
    frames = RS.frames_of(sc, dev)
    Hv, Wv, r = 240, 320, ps // 2
    _, d1, i1 = draw(frames, view, Kc, (Hv, Wv), dev, near=NEAR)
    _, ds, is_ = draw(frames, view, Kc, (Hv, Wv), dev, near=NEAR, point_size=ps)
    k1 = np.full((Hv + 2 * r, Wv + 2 * r), np.uint64(0xffffffffffffffff))
    k1[r:r + Hv, r:r + Wv] = keys_of(d1, i1)
    want = np.full((Hv, Wv), np.uint64(0xffffffffffffffff))
    for oy in range(2 * r + 1):
        for ox in range(2 * r + 1):
            want = np.minimum(want, k1[oy:oy + Hv, ox:ox + Wv])
    got = keys_of(ds, is_)
    # a window that lies inside the image sees every source that can reach its pixel: an identity.  Within r pixels of
    # the border a source whose centre is outside the image may also have written: the key can only be smaller.
    assert np.array_equal(got[r:Hv - r, r:Wv - r], want[r:Hv - r, r:Wv - r])
    assert (got <= want).all()
    assert (is_ >= 0).sum() > (i1 >= 0).sum()


# ---- 4. consistency with the export ----------------------------------------------------------------------------------
def test_rendered_depth_is_the_exported_point_seen_from_the_camera(dev):
    sc = RS.general_scene(3, 128, 256, seed=6, layout="f32")
    view, Kc = RS.general_view((240, 320), "back")
    frames = RS.frames_of(sc, dev)
    _, depth, index = draw(frames, view, Kc, (240, 320), dev, near=NEAR, c_conf_threshold=None)
    p, _, i = export.collect_map(frames, c_conf_threshold=None, return_index=True)
    p, i = p.cpu().numpy(), i.cpu().numpy()
    hit = index >= 0
    row = np.searchsorted(i, index[hit])
    assert np.array_equal(i[row], index[hit])                                # every rendered source is an exported one
    Rt, t, inv_s = RT.view_inverse(view)
    z = ((p[row].astype(np.float64) - t) @ Rt.T)[:, 2] * inv_s
    rel = np.abs(depth[hit].astype(np.float64) - z) / z
    print(f"{int(hit.sum())} pixels, max relative |depth - z(exported point)| = {rel.max():.3g}")
    assert (rel <= 1e-5).all()
    # with the identity view the camera transform is exact: depth is the exporter's world z, bit for bit
    ident = np.array([0, 0, 0, 0, 0, 0, 1, 1], dtype=np.float32)
    _, depth, index = draw(frames, ident, Kc, (240, 320), dev, near=NEAR, c_conf_threshold=None)
    hit = index >= 0
    row = np.searchsorted(i, index[hit])
    assert hit.sum() > 1000 and depth[hit].tobytes() == np.ascontiguousarray(p[row, 2]).tobytes()


# ---- 5. determinism, graph capture, empty views, many keyframes ----------------------------------------------------
def test_two_calls_give_identical_bytes(dev):
    sc = RS.general_scene(3, 128, 256, seed=8, layout="u8")
    frames = RS.frames_of(sc, dev)
    view, Kc = RS.general_view((240, 320), "back")
    far_view = view.copy()
    far_view[2] -= 400.0                                                     # the whole map in a few pixels: contention
    for v, ps in ((view, 1), (view, 7), (far_view, 1), (far_view, 3)):
        a = draw(frames, v, Kc, (240, 320), dev, near=NEAR, point_size=ps, c_conf_threshold=None)
        b = draw(frames, v, Kc, (240, 320), dev, near=NEAR, point_size=ps, c_conf_threshold=None)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and (a[2] >= 0).any()
    assert (draw(frames, far_view, Kc, (240, 320), dev, near=NEAR, c_conf_threshold=None)[2] >= 0).sum() < 64


def test_graph_replay_reads_the_pose_on_the_device(dev):
    sc = RS.general_scene(3, 128, 256, seed=10, layout="u8")
    frames = RS.frames_of(sc, dev)
    size = (240, 320)
    va, Kc = RS.general_view(size, "inside")
    vb, _ = RS.general_view(size, "back", seed=3)
    want_a, want_b = (draw(frames, v, Kc, size, dev, near=NEAR) for v in (va, vb))
    assert want_a[2].tobytes() != want_b[2].tobytes()
    pose = torch.from_numpy(va).to(dev)
    out = (torch.empty((*size, 3), dtype=torch.uint8, device=dev), torch.empty(size, dtype=torch.float32, device=dev),
           torch.empty(size, dtype=torch.int64, device=dev))
    ws = torch.empty(render.workspace_bytes(size), dtype=torch.uint8, device=dev)
    tables = render.map_tables(frames)                                       # host-to-device copies stay outside the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                            # warm-up outside the capture
        render.render_map(tables, pose, Kc, size, near=NEAR, return_index=True, out=out, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        render.render_map(tables, pose, Kc, size, near=NEAR, return_index=True, out=out, workspace=ws)
    for o in out:
        o.zero_()
    graph.replay()
    assert all(o.cpu().numpy().tobytes() == w.tobytes() for o, w in zip(out, want_a))
    pose.copy_(torch.from_numpy(vb).to(dev))                                 # in place: the graph holds the address
    graph.replay()
    assert all(o.cpu().numpy().tobytes() == w.tobytes() for o, w in zip(out, want_b))


def test_a_view_that_sees_nothing_and_an_empty_map_give_the_background(dev):
    sc = RS.general_scene(1, 1, 4999, seed=12, layout="u8")
    frames = RS.frames_of(sc, dev)
    view, Kc = RS.general_view((48, 64), "inside")
    away = view.copy()
    away[3:7] = [0, 1, 0, 0]                                                 # half a turn about y: the map is behind the camera
    pose = torch.from_numpy(view).to(dev)
    for kfs, v in ((frames, away), ([], view)):
        rgb, depth, index = draw(kfs, v, Kc, (48, 64), dev, background=(9, 8, 7))
        assert (rgb == (9, 8, 7)).all() and np.isposinf(depth).all() and (index == -1).all()
    assert len(render.render_map([], pose, None, (48, 64))) == 2


def test_256_small_keyframes_in_three_launches(dev):
    L = _ffi.lib()
    assert L.m3_render_launches(256) == L.m3_render_launches(1) == 3        # the entry point's documented launch count
    sc = RS.general_scene(256, 16, 24, seed=14, layout="u8")
    view, Kc = RS.general_view((240, 320), "inside")
    tw = RT.render_twin(sc, view, Kc, (240, 320), near=NEAR)
    rgb, depth, index = draw(RS.frames_of(sc, dev), view, Kc, (240, 320), dev, near=NEAR)
    RT.check_against_twin(tw, rgb, depth, index, "K=256 16x24 -> 240x320")
    assert np.unique(index[index >= 0] // (16 * 24)).size > 200              # most keyframes are visible
