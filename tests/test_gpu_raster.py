"""GPU: the triangle rasteriser (csrc/raster.hip through render.render_mesh) against its twin (tests/raster_twin.py).

Exact scenes (raster_scenes.exact: every fp32 step of the vertex stage is exact) must match the twin's fp32 emulation
bit for bit.  General scenes must match the float64 twin on every uncontested pixel (index exactly, depth within the
per-face bound, colour within 1) and give -1 or a face that covers the pixel on a contested one; a scene whose contested
pixels exceed 5 % of its covered pixels fails as untestable."""
import gc

import numpy as np
import pytest
import torch

import raster_scenes as RS
import raster_twin as RW
import render_scenes as PS
import render_twin as RT
from mast3r_slam import _ffi, export, render, synthetic

pytestmark = pytest.mark.gpu


def on(sc, dev):
    return (torch.from_numpy(sc["vertices"]).to(dev), torch.from_numpy(sc["colors"]).to(dev), torch.from_numpy(sc["faces"]).to(dev))


def draw(sc, dev, mesh=None, **kw):
    view = torch.from_numpy(np.asarray(sc["view"], dtype=np.float32)).to(dev)
    rgb, depth, index = render.render_mesh(*(mesh or on(sc, dev)), view, sc["K"], sc["size"], return_index=True, **dict(sc["kw"], **kw))
    assert rgb.dtype == torch.uint8 and depth.dtype == torch.float32 and index.dtype == torch.int64
    return rgb.cpu().numpy(), depth.cpu().numpy(), index.cpu().numpy()


def twin(sc, **kw):
    return RW.raster_twin(sc["vertices"], sc["colors"], sc["faces"], sc["view"], sc["K"], sc["size"], **dict(sc["kw"], **kw))


# ---- 1. exact scenes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,offset,shared", RS.EXACT)
def test_exact_scenes_are_byte_equal(dev, size, offset, shared):
    sc = RS.exact(size, offset, 3, shared)
    for cull in ("none", "back"):
        want = RW.fp32_emulation(sc["vertices"], sc["colors"], sc["faces"], sc["view"], sc["K"], sc["size"], **dict(sc["kw"], cull=cull))
        rgb, depth, index = draw(sc, dev, cull=cull)
        print(f"{size} offset {offset} shared {shared} cull {cull}: {int((index >= 0).sum())} of {index.size} pixels covered, "
              f"{np.unique(index).size} faces seen")
        assert (index >= 0).all() and np.array_equal(index, want[2])
        assert depth.tobytes() == want[1].tobytes()
        assert np.array_equal(rgb, want[0])                                  # shared False: one colour per face
    assert ((index < sc["originals"]) | (index == len(sc["faces"]) - 1)).all()   # equal depths went to the smaller index


# ---- 2. general scenes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RS.GENERAL)
def test_general_scenes_against_the_twin(dev, name):
    sc = RS.general(name)
    tw = twin(sc)
    RW.check_against_twin(tw, *draw(sc, dev), name)
    assert tw["covered"].sum() > 1000
    if name == "near_third":
        behind = ~RW.vertex_stage(sc["vertices"], sc["view"], sc["K"], sc["kw"]["near"], np.inf)["ok"]
        assert abs(behind.mean() - 1 / 3) < 0.02


# ---- 3. the wave's path ------------------------------------------------------------------------------------------------
def test_a_screen_filling_quad_behind_small_faces(dev):
    sc = RS.large_quad_behind_sheet()
    tw = twin(sc)
    rgb, depth, index = draw(sc, dev)
    RW.check_against_twin(tw, rgb, depth, index, "large quad")
    assert (index >= 0).all() and (index < 2).sum() > 6000 and (index >= 2).sum() > 1000


def test_a_subdivided_sheet_gives_the_image_of_the_sheet(dev):
    sc = RS.planar_sheet()
    sub = RS.subdivided(sc)
    assert RS.box_pixels(sc).min() > 64 and RS.box_pixels(sub).max() <= 64    # the wave's path against the lane's
    ta, tb = twin(sc), twin(sub)
    a, b = draw(sc, dev), draw(sub, dev)
    RW.check_against_twin(ta, *a, "planar sheet")
    assert RW.check_same_surface(ta, a, tb, b, "subdivided against coarse") > 1000


def test_a_single_face_over_a_256_view(dev):
    sc = RS.single_face()
    rgb, depth, index = draw(sc, dev)
    RW.check_against_twin(twin(sc), rgb, depth, index, "single face")
    assert (index == 0).all()


# ---- 4. bad indices and degenerate faces ---------------------------------------------------------------------------------
def test_bad_indices_are_skipped_and_degenerate_faces_draw_nothing(dev):
    sc = RS.general("front")
    V, F = len(sc["vertices"]), sc["faces"]
    want = draw(sc, dev)
    junk = np.array([[-1, 0, 1], [0, V, 1], [0, 1, 2 ** 31 - 1], [-2 ** 31, 5, 6], [V, V + 1, V + 2], [3, 3, 4], [7, 8, 7],
                     [9, 9, 9]], dtype=np.int32)
    pos = np.arange(len(F)) + np.minimum(np.arange(len(F)) // 60 + 1, len(junk))   # a junk face before every 60th valid one
    mixed = np.empty((len(F) + len(junk), 3), dtype=np.int32)
    mixed[pos] = F
    mixed[np.setdiff1d(np.arange(len(mixed)), pos)] = junk
    back = np.full(len(mixed), -1, dtype=np.int64)
    back[pos] = np.arange(len(F))
    rgb, depth, index = draw(dict(sc, faces=mixed), dev)                       # returns: the call's status was M3_OK
    assert depth.tobytes() == want[1].tobytes() and rgb.tobytes() == want[0].tobytes()
    assert np.array_equal(np.where(index >= 0, back[index], -1), want[2]) and (want[2] >= 0).sum() > 1000
    only_junk = draw(dict(sc, faces=junk), dev)
    assert (only_junk[2] == -1).all() and np.isposinf(only_junk[1]).all()


# ---- 5. culling ----------------------------------------------------------------------------------------------------------
def keyframe(dev, h=48, w=64):
    """A synthetic keyframe (synthetic._surface: the pinhole f = w, principal point (w / 2, h / 2)) at a general pose."""
    vv, uu = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    X = synthetic._surface(uu, vv, h, w).reshape(-1, 3).astype(np.float32)
    T = RS._pose([0.3, -0.2, 0.1], [0.1, -0.2, 0.05], 1.25)
    img = synthetic.textured_image(h, w, 3).reshape(1, h * w, 3)
    sc = dict(X=X[None], C=np.full((1, h * w), 2.0, dtype=np.float32), Nk=np.array([1], dtype=np.int32), T=T[None], img=img,
              layout="u8", K=1, N=h * w, H=h, W=w)
    return PS.frames_of(sc, dev), T, (float(w), float(w), w / 2.0, h / 2.0)


def test_cull_back(dev):
    sc = RS.general("mixed")
    tw = twin(sc, cull="back")
    rgb, depth, index = draw(sc, dev, cull="back")
    RW.check_against_twin(tw, rgb, depth, index, "mixed windings, cull back")
    assert 1000 < tw["covered"].sum() < twin(sc)["covered"].sum()
    # collect_mesh's faces are counter-clockwise seen from their keyframe: culling keeps all of them
    frames, T, Kc = keyframe(dev)
    mesh = export.collect_mesh(frames, edge_ratio=0.2)
    pose = torch.from_numpy(T).to(dev)
    none = render.render_mesh(mesh, pose, Kc, (48, 64), return_index=True)
    back = render.render_mesh(mesh, pose, Kc, (48, 64), return_index=True, cull="back")
    assert all(torch.equal(a, b) for a, b in zip(none, back)) and (none[2] >= 0).sum() > 2500
    flipped = (mesh[0], mesh[1], mesh[2][:, [0, 2, 1]].contiguous())
    assert (render.render_mesh(flipped, pose, Kc, (48, 64), return_index=True, cull="back")[2] == -1).all()


# ---- 6. agreement with the point renderer --------------------------------------------------------------------------------
def test_mesh_depth_agrees_with_the_point_view_and_fills_its_holes(dev):
    h, w = 48, 64
    frames, T, Kc = keyframe(dev, h, w)
    pose = torch.from_numpy(T).to(dev)
    mesh = export.collect_mesh(frames, edge_ratio=0.2)
    assert mesh[0].shape[0] == h * w                                           # every point is a vertex
    _, dm, im = (t.cpu().numpy() for t in render.render_mesh(mesh, pose, Kc, (h, w), return_index=True))
    _, dp, ip = (t.cpu().numpy() for t in render.render_map(frames, pose, Kc, (h, w), return_index=True))
    both = (im >= 0) & (ip >= 0)
    # a point lands on the pixel centre up to the fp32 round trip through the pose, its vertex within a step of that:
    # the bound of a one-step vertex move on the winning face, plus the point renderer's own
    V, F = mesh[0].cpu().numpy(), mesh[2].cpu().numpy()
    vs = RW.vertex_stage(V, T, Kc, 1e-3, np.inf)
    bound = RW.face_bounds(vs, F)[im[both]] + RT.DEPTH_RTOL
    rel = np.abs(dm[both].astype(np.float64) - dp[both]) / dp[both]
    print(f"{int(both.sum())} pixels drawn by both, max relative depth difference {rel.max():.3g}, smallest bound {bound.min():.3g}")
    assert both.sum() > 2500 and (rel <= bound).all()
    # twice the size: the points leave three pixels in four empty, the mesh none inside the silhouette
    size2 = (2 * h, 2 * w)
    K2 = render.scaled_intrinsics(Kc, (h, w), size2)
    im2 = render.render_mesh(mesh, pose, K2, size2, return_index=True)[2].cpu().numpy()
    ip2 = render.render_map(frames, pose, K2, size2, return_index=True)[2].cpu().numpy()
    inside = np.zeros(size2, dtype=bool)
    inside[2:-3, 2:-3] = True                                                  # vertex (x, y) lands on pixel (2 x + 0.5, 2 y + 0.5)
    holes = inside & (ip2 < 0)
    print(f"2x view: the point view leaves {int(holes.sum())} of {int(inside.sum())} pixels inside the silhouette empty")
    assert holes.sum() > inside.sum() // 2 and (im2[holes] >= 0).all() and (im2[inside] >= 0).all()


# ---- 7. determinism and allocation -----------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes_and_reuse_allocates_nothing(dev):
    for sc in (RS.general("front"), RS.large_quad_behind_sheet()):
        a, b = draw(sc, dev), draw(sc, dev)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and (a[2] >= 0).any()
        mesh = on(sc, dev)
        view = torch.from_numpy(sc["view"]).to(dev)
        size = sc["size"]
        out = (torch.empty((*size, 3), dtype=torch.uint8, device=dev), torch.empty(size, dtype=torch.float32, device=dev),
               torch.empty(size, dtype=torch.int64, device=dev))
        ws = torch.empty(render.mesh_workspace_bytes(len(sc["vertices"]), size), dtype=torch.uint8, device=dev)
        gc.collect()                                                           # nothing of the calls above is freed meanwhile
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        got = render.render_mesh(*mesh, view, sc["K"], size, return_index=True, out=out, workspace=ws, **sc["kw"])
        assert torch.cuda.max_memory_allocated(dev) == before                  # the peak never rose: nothing was allocated
        assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
        assert all(o.cpu().numpy().tobytes() == x.tobytes() for o, x in zip(out, a))
        with pytest.raises(ValueError, match="workspace"):
            render.render_mesh(*mesh, view, sc["K"], size, workspace=ws[:-16], **sc["kw"])


# ---- 8. graph capture --------------------------------------------------------------------------------------------------
def test_graph_replay_reads_the_pose_on_the_device(dev):
    sa, sb = RS.general("front"), RS.general("oblique")                        # the same mesh from two poses
    want_a, want_b = draw(sa, dev), draw(sb, dev)
    assert want_a[2].tobytes() != want_b[2].tobytes()
    mesh, size = on(sa, dev), sa["size"]
    pose = torch.from_numpy(sa["view"]).to(dev)
    out = (torch.empty((*size, 3), dtype=torch.uint8, device=dev), torch.empty(size, dtype=torch.float32, device=dev),
           torch.empty(size, dtype=torch.int64, device=dev))
    ws = torch.empty(render.mesh_workspace_bytes(len(sa["vertices"]), size), dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                            # warm-up outside the capture
        render.render_mesh(*mesh, pose, sa["K"], size, return_index=True, out=out, workspace=ws, **sa["kw"])
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        render.render_mesh(*mesh, pose, sa["K"], size, return_index=True, out=out, workspace=ws, **sa["kw"])
    for o in out:
        o.zero_()
    graph.replay()
    assert all(o.cpu().numpy().tobytes() == w.tobytes() for o, w in zip(out, want_a))
    pose.copy_(torch.from_numpy(sb["view"]).to(dev))                           # in place: the graph holds the address
    graph.replay()
    assert all(o.cpu().numpy().tobytes() == w.tobytes() for o, w in zip(out, want_b))


# ---- 9. empty and invisible ----------------------------------------------------------------------------------------------
def test_empty_meshes_and_a_mesh_behind_the_camera_give_the_background(dev):
    L = _ffi.lib()
    assert L.m3_raster_launches(0) == 2 and L.m3_raster_launches(1) == L.m3_raster_launches(10 ** 9) == 4
    sc = RS.general("front")
    away = sc["view"].copy()
    away[3:7] = [0, 1, 0, 0]                                                   # half a turn about y: the mesh is behind the camera
    none_v = dict(sc, vertices=np.zeros((0, 3), np.float32), colors=np.zeros((0, 3), np.uint8))
    none_f = dict(sc, faces=np.zeros((0, 3), np.int32))
    for s in (dict(sc, view=away), none_f, dict(none_v, faces=np.zeros((0, 3), np.int32)), none_v):
        rgb, depth, index = draw(s, dev, background=(9, 8, 7))
        assert (rgb == (9, 8, 7)).all() and np.isposinf(depth).all() and (index == -1).all()
    pose = torch.from_numpy(sc["view"]).to(dev)
    assert len(render.render_mesh(export._empty_mesh(dev, False), pose, None, (48, 64))) == 2


# ---- 10. unaligned outputs -------------------------------------------------------------------------------------------------
def test_unaligned_outputs_take_the_scalar_path(dev):
    sc = RS.general("front")
    ref = draw(sc, dev)
    Hv, Wv = sc["size"]
    P = Hv * Wv
    out = (torch.empty(3 * P + 1, dtype=torch.uint8, device=dev)[1:].view(Hv, Wv, 3),
           torch.empty(P + 1, dtype=torch.float32, device=dev)[1:].view(Hv, Wv),
           torch.empty(P + 1, dtype=torch.int64, device=dev)[1:].view(Hv, Wv))
    assert out[0].data_ptr() % 4 and out[1].data_ptr() % 16 and out[2].data_ptr() % 16
    got = draw(sc, dev, out=out)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ref, got))
    odd = RS.odd_size()
    RW.check_against_twin(twin(odd), *draw(odd, dev), "61 x 83")
