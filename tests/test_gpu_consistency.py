"""GPU: the multi-view consistency filter (csrc/consistency.hip through consistency.multiview_support) against its
float64 twin (tests/consistency_twin.py).

The exact scene (every fp32 operation of the rule is exact) must match the twin byte for byte.  Shared scenes must match
it on every uncontested source and stay within the number of contested pairs on a contested one; a scene with more than
5 % contested candidates fails as untestable.  Neighbour selection, determinism, the launch count, graph capture and the
integration with the exporters are exact."""
import ctypes

import numpy as np
import pytest
import torch

import consistency_twin as CT
import render_scenes as RS
from mast3r_slam import _ffi, consistency, export, render

pytestmark = pytest.mark.gpu


def run(frames, pin, **kw):
    s, c, conf = consistency.multiview_support(frames, pin, **kw)
    assert s.dtype == torch.uint8 and c.dtype == torch.uint8 and conf.dtype == torch.float32 and s.is_cuda
    return s.cpu().numpy(), c.cpu().numpy(), conf.cpu().numpy()


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- 1. exact scene, hand-made case ----------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["f32", "u8"])
def test_exact_scene_is_byte_equal(dev, layout):
    sc, pin, nbr = CT.exact_scene(5, layout)
    assert sc["K"] == 4 and sc["N"] == 33 * 65
    frames = RS.frames_of(sc, dev)
    table = torch.from_numpy(nbr).to(dev)
    for thr in (1.5, None):
        for mv, mc in CT.RULES:
            kw = dict(z_min=CT.EXACT_ZMIN, depth_rtol=CT.EXACT_RTOL, min_views=mv, max_conflicts=mc)
            tw = CT.twin(sc, pin, nbr, thr=thr, **kw)
            s, c, conf = run(frames, pin, neighbours=table, c_conf_threshold=thr, **kw)
            print(f"{layout} thr={thr} rule=({mv}, {mc}): {int(tw['cand'].sum())} candidates, {int(tw['support'].sum())} agreements, "
                  f"{int(tw['conflict'].sum())} conflicts, {int(tw['kept'].sum())} kept")
            assert np.array_equal(s, tw["support"]) and np.array_equal(c, tw["conflict"])
            assert conf.tobytes() == tw["conf"].tobytes()
    for m, (d, cz) in sc["ulp"].items():                                      # one ulp past the boundary does not agree
        assert s[0, m] == 0 and c[0, m] == (1 if cz < d else 0)


def test_hand_made_case(dev):
    sc, pin, support, conflict = CT.hand_case()
    s, c, conf = run(RS.frames_of(sc, dev), pin, neighbours=None, min_views=1, max_conflicts=1)
    assert np.array_equal(s, support) and np.array_equal(c, conflict)
    kept = np.array([[1, 1, 0, 0], [1, 1, 1, 0], [1, 0, 1, 0]], dtype=bool)
    assert np.array_equal(conf, np.where(kept, sc["C"], -np.inf).astype(np.float32))


# ---- 2. shared scenes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,H,W,seed", CT.SHARED)
def test_shared_scenes_against_the_twin(dev, K, H, W, seed):
    sc = CT.shared_scene(K, H, W, seed, layout="u8" if K % 2 else "f32")
    pin = CT.shared_pinhole(H, W)
    frames = RS.frames_of(sc, dev)
    aligned = all(f.X_canon.data_ptr() % 16 == 0 and f.C.data_ptr() % 16 == 0 for f in frames) and (H * W) % 4 == 0
    assert aligned == (K == 4)                                               # 64 x 128 takes the 16-byte loads, 33 x 65 the scalar ones
    for label, nbr, arg in CT.tables_of(sc):
        arg = torch.from_numpy(nbr).to(dev) if isinstance(arg, str) else arg
        for mv, mc in CT.RULES:
            tw = CT.twin(sc, pin, nbr, min_views=mv, max_conflicts=mc)
            s, c, conf = run(frames, pin, neighbours=arg, min_views=mv, max_conflicts=mc)
            CT.check_against_twin(tw, sc, s, c, conf, mv, mc, f"{K}x{H}x{W} {label} rule=({mv}, {mc})")
        if label == "explicit":
            assert (s[K - 1] == 0).all() and (c[K - 1] == 0).all()            # a row of only -1
    tw = CT.twin(sc, pin, CT.all_others(K), thr=None)
    CT.check_against_twin(tw, sc, *run(frames, pin, neighbours=None, c_conf_threshold=None), 2, 1, f"{K}x{H}x{W} all thr=None")


def test_unaligned_keyframes_give_the_same_bytes(dev):
    K, H, W, seed = CT.SHARED[1]
    sc = CT.shared_scene(K, H, W, seed)
    pin = CT.shared_pinhole(H, W)
    frames = RS.frames_of(sc, dev)
    ref = run(frames, pin, neighbours=None)
    for f in frames[::2]:
        for name in ("X_canon", "C"):
            t = getattr(f, name)
            buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
            buf[1:] = t.reshape(-1)
            setattr(f, name, buf[1:].view(t.shape))
            assert getattr(f, name).data_ptr() % 16 != 0
    assert same_bytes(ref, run(frames, pin, neighbours=None))


# ---- 3. neighbour selection ------------------------------------------------------------------------------------------
def test_nearest_neighbours_equal_a_stable_argsort(dev):
    sc = CT.shared_scene(5, 33, 65, 15, grid_centres=True)                    # camera centres on a 1/8 grid: exact distances, ties
    pin = CT.shared_pinhole(33, 65)
    frames = RS.frames_of(sc, dev)
    d2 = ((sc["T"][:, None, :3] - sc["T"][None, :, :3]).astype(np.float64) ** 2).sum(axis=2)
    assert any(np.unique(row).size < row.size for row in d2)                  # at least one tie: stability matters
    for v in (1, 3, 8):
        nbr = CT.nearest(sc["T"], v)
        got = consistency.nearest_neighbours(torch.from_numpy(sc["T"]).to(dev), v)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), nbr) and nbr.shape == (5, min(v, 4))
        assert same_bytes(run(frames, pin, neighbours=v), run(frames, pin, neighbours=torch.from_numpy(nbr).to(dev)))
    tw = CT.twin(sc, pin, CT.nearest(sc["T"], 3))
    CT.check_against_twin(tw, sc, *run(frames, pin, neighbours=3), 2, 1, "grid centres nearest3")


def test_a_single_keyframe_has_no_support(dev):
    sc = CT.shared_scene(1, 33, 65, 14)
    pin = CT.shared_pinhole(33, 65)
    frames = RS.frames_of(sc, dev)
    for nb in (None, 8, torch.tensor([[0]], dtype=torch.int32, device=dev)):
        s, c, conf = run(frames, pin, neighbours=nb, min_views=1)
        assert not s.any() and not c.any() and np.isneginf(conf).all()
        s, c, conf = run(frames, pin, neighbours=nb, min_views=0)
        assert not s.any() and not c.any()
        _, _, index = export.collect_map(frames, return_index=True)           # the exporter's candidates
        kept = np.zeros(sc["N"], dtype=bool)
        kept[index.cpu().numpy()] = True
        assert conf.tobytes() == np.where(kept, sc["C"][0], np.float32(-np.inf)).astype(np.float32).tobytes() and kept.any()


# ---- 4. determinism, locality, launches, capture ------------------------------------------------------------------
def test_identical_bytes_and_a_keyframe_depends_on_its_neighbours_only(dev):
    K, H, W, seed = CT.SHARED[2]
    sc = CT.shared_scene(K, H, W, seed)
    pin = CT.shared_pinhole(H, W)
    frames = RS.frames_of(sc, dev)
    nbr = CT.nearest(sc["T"], 2)
    table = torch.from_numpy(nbr).to(dev)
    a, b = run(frames, pin, neighbours=table), run(frames, pin, neighbours=table)
    assert same_bytes(a, b) and a[0].any() and a[1].any()
    for k in range(K):
        members = [k] + [int(j) for j in nbr[k]]                              # renumbered: 0 is k, then its neighbours
        sub = torch.tensor([[1, 2], [-1, -1], [-1, -1]], dtype=torch.int32, device=dev)
        got = run([frames[i] for i in members], pin, neighbours=sub)
        assert all(x[0].tobytes() == y[k].tobytes() for x, y in zip(got, a))


def raw_call(L, m, pin, nbr, out, ws, hw, stream):
    poses = m.poses
    return L.m3_consistency(_ffi.ptr(m.table[0]), _ffi.ptr(m.table[1]), _ffi.ptr(poses), _ffi.ptr(m.nk), m.k, hw[0], hw[1], 1, 1.5,
                            *pin, _ffi.ptr(nbr), int(nbr.shape[1]), 1e-3, 0.03, 2, 1, _ffi.ptr(ws), ws.numel(),
                            _ffi.ptr(out[0]), _ffi.ptr(out[1]), _ffi.ptr(out[2]), stream)


@pytest.mark.parametrize("K", [1, 5])
def test_launch_count_is_the_documented_constant(dev, K):
    """The launches the entry point queues are counted as the nodes of a stream capture of one call (captured, never
    replayed), through the HIP runtime the library itself is linked against."""
    L = _ffi.lib()
    H, W = 33, 65
    sc = CT.shared_scene(K, H, W, 20 + K)
    pin = CT.shared_pinhole(H, W)
    frames = RS.frames_of(sc, dev)
    m = render.map_tables(frames)
    nbr = torch.from_numpy(CT.all_others(K) if K > 1 else np.array([[-1]], dtype=np.int32)).to(dev)
    out = (torch.empty((K, H * W), dtype=torch.uint8, device=dev), torch.empty((K, H * W), dtype=torch.uint8, device=dev),
           torch.empty((K, H * W), dtype=torch.float32, device=dev))
    ws = torch.empty(consistency.workspace_bytes(K, H * W), dtype=torch.uint8, device=dev)
    want = run(frames, pin, neighbours=nbr)
    hip = ctypes.CDLL(_ffi.LIB_PATH)                                         # dlsym also searches the library's dependencies
    for name in ("hipStreamBeginCapture", "hipStreamEndCapture", "hipGraphGetNodes", "hipGraphDestroy"):
        getattr(hip, name).restype = ctypes.c_int
    hip.hipStreamBeginCapture.argtypes = [ctypes.c_void_p, ctypes.c_int]
    hip.hipStreamEndCapture.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    hip.hipGraphDestroy.argtypes = [ctypes.c_void_p]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph, nodes = ctypes.c_void_p(), ctypes.c_size_t(0)
    assert hip.hipStreamBeginCapture(side.cuda_stream, 2) == 0               # hipStreamCaptureModeRelaxed
    rc = raw_call(L, m, pin, nbr, out, ws, (H, W), side.cuda_stream)
    assert hip.hipStreamEndCapture(side.cuda_stream, ctypes.byref(graph)) == 0 and rc == 0
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(nodes)) == 0
    assert hip.hipGraphDestroy(graph) == 0
    print(f"K={K}: {nodes.value} graph nodes for one call")
    assert nodes.value == L.m3_consistency_launches() == 3
    assert raw_call(L, m, pin, nbr, out, ws, (H, W), _ffi.stream_ptr()) == 0  # the same arguments, run: the eager result
    assert same_bytes([o.cpu().numpy() for o in out], want)


def test_graph_replay_reads_the_poses_on_the_device(dev):
    K, H, W, seed = CT.SHARED[0]
    sc = CT.shared_scene(K, H, W, seed)
    pin = CT.shared_pinhole(H, W)
    frames = RS.frames_of(sc, dev)
    nbr = torch.from_numpy(CT.all_others(K)).to(dev)
    new_pose = sc["T"][1].copy()
    new_pose[:3] += np.float32([0.05, -0.02, 0.08])
    new_pose[7] *= np.float32(1.02)
    want_a = run(frames, pin, neighbours=nbr)
    out = (torch.empty((K, H * W), dtype=torch.uint8, device=dev), torch.empty((K, H * W), dtype=torch.uint8, device=dev),
           torch.empty((K, H * W), dtype=torch.float32, device=dev))
    ws = torch.empty(consistency.workspace_bytes(K, H * W), dtype=torch.uint8, device=dev)
    tables = render.map_tables(frames)                                       # host-to-device copies stay outside the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                            # warm-up outside the capture
        consistency.multiview_support(tables, pin, neighbours=nbr, out=out, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                             # one stream: a serial chain of launches
        consistency.multiview_support(tables, pin, neighbours=nbr, out=out, workspace=ws)
    for o in out:
        o.zero_()
    graph.replay()
    assert same_bytes([o.cpu().numpy() for o in out], want_a)
    frames[1].T_WC.copy_(torch.from_numpy(new_pose).to(dev).reshape(1, 8))   # in place: the graph reads this tensor
    graph.replay()
    got_b = [o.cpu().numpy() for o in out]
    want_b = run(frames, pin, neighbours=nbr)                                 # eager, on the new pose
    assert same_bytes(got_b, want_b) and not same_bytes(want_a, want_b)


# ---- 5. integration with the exporters -------------------------------------------------------------------------------
def test_consistent_keyframes_filter_the_map_and_the_mesh(dev):
    K, H, W, seed = CT.SHARED[1]
    sc = CT.shared_scene(K, H, W, seed, layout="f32")
    pin = CT.shared_pinhole(H, W)
    frames = RS.frames_of(sc, dev, shape=(H, W))
    before = [(f.C.clone(), f.C.data_ptr()) for f in frames]
    _, _, conf = run(frames, pin, neighbours=None)
    kept = ~np.isneginf(conf)
    idx = np.nonzero(kept.reshape(-1))[0]                                     # k * N + n of the kept points
    views = consistency.consistent_keyframes(frames, pin, neighbours=None)
    assert [v.frame_id for v in views] == [f.frame_id for f in frames]
    assert all(v.X_canon is f.X_canon and v.T_WC is f.T_WC and v.img is f.img and v.N == f.N for v, f in zip(views, frames))
    assert all(torch.equal(f.C.view(torch.int32), c.view(torch.int32)) and f.C.data_ptr() == p for f, (c, p) in zip(frames, before))   # untouched
    p, col, index0 = (t.cpu().numpy() for t in export.collect_map(frames, return_index=True))
    pf, colf, indexf = (t.cpu().numpy() for t in export.collect_map(views, return_index=True))
    print(f"{index0.size} exported points, {indexf.size} after the filter")
    assert 0 < indexf.size < index0.size
    assert np.array_equal(indexf, idx)
    sel = np.isin(index0, idx)
    assert pf.tobytes() == p[sel].tobytes() and colf.tobytes() == col[sel].tobytes()
    for thr in (0.5, -np.inf):                                               # any other finite threshold, or "every kept point"
        assert np.array_equal(export.collect_map(views, c_conf_threshold=thr, return_index=True)[2].cpu().numpy(), idx)
    v, _, faces, vi = (t.cpu().numpy() for t in export.collect_mesh(views, edge_ratio=0.2, return_index=True))
    assert faces.shape[0] > 0 and np.isin(vi, idx).all() and faces.max() < v.shape[0]
    v0 = export.collect_mesh(frames, edge_ratio=0.2)[0]
    assert v.shape[0] < v0.shape[0]
    rgb, depth, ri = render.render_map(views, frames[0].T_WC, pin, (H, W), return_index=True)
    ri = ri.cpu().numpy()
    assert (ri >= 0).any() and np.isin(ri[ri >= 0], idx).all()
