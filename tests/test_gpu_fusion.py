"""GPU: the volumetric fusion (csrc/tsdf.hip through fusion.fuse_tsdf / extract_surface) against its twins
(tests/tsdf_twin.py).

Integration: byte-equal to the float32 twin on every voxel; against the float64 twin, equal weights and colours and
|tsdf - twin| <= tsdf_tolerance on uncontested voxels, weights within the number of contested pairs elsewhere; a volume
with more than 5 % contested voxels fails as untestable.  Extraction: faces and colours equal the twin's, vertices
byte-equal to the float32 twin's.  Determinism, the launch counts, graph capture and the consistency views are exact."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import consistency_twin as CT
import render_scenes as RS
import tsdf_twin as TT
from mast3r_slam import _ffi, consistency, fusion, render

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def scene(K, H, W, seed, layout="u8"):
    return CT.shared_scene(K, H, W, seed, layout=layout)


@functools.lru_cache(maxsize=None)
def twins(K, H, W, seed, layout, thr):
    """(float64 twin, float32 twin) of a shared scene in the test volume: computed once, never modified."""
    sc, pin, vol = scene(K, H, W, seed, layout), CT.shared_pinhole(H, W), TT.VOLUME
    return TT.integrate(sc, pin, vol, thr=thr), TT.integrate(sc, pin, vol, thr=thr, dtype=np.float32)


def out_of(vol, dev):
    return fusion.empty_volume(vol["origin"], vol["dims"], vol["vs"], vol["trunc"], dev)


def fuse(frames, pin, vol, dev, **kw):
    v = fusion.fuse_tsdf(frames, pin, vol["vs"], trunc=vol["trunc"], out=out_of(vol, dev), **kw)
    assert v.tsdf.is_cuda and v.dims == vol["dims"]
    return v


def host(v):
    return v.tsdf.cpu().numpy(), v.weight.cpu().numpy(), v.color.cpu().numpy(), v.colored.cpu().numpy()


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def mesh_host(mesh):
    return tuple(t.cpu().numpy() for t in mesh)


def check_extraction(volume, arrays, min_weight=1, label=""):
    """extract_surface of a device volume against the twin run on the same arrays."""
    v, c, f = mesh_host(fusion.extract_surface(volume, min_weight=min_weight))
    tv, tc, tf = TT.extract(*arrays, volume.origin, volume.voxel_size, min_weight=min_weight, dtype=np.float32)
    tv64 = TT.extract(*arrays, volume.origin, volume.voxel_size, min_weight=min_weight)[0]
    print(f"{label} min_weight={min_weight}: {tv.shape[0]} vertices, {tf.shape[0]} faces; device {v.shape[0]}, {f.shape[0]}; "
          f"f32 twin against f64 {float(np.abs(tv - tv64).max()) if tv.size else 0.0:.3g}")
    assert v.dtype == np.float32 and c.dtype == np.uint8 and f.dtype == np.int32
    if tf.shape[0] == 0:                                                       # no face: the mesh is empty
        assert v.shape == (0, 3) and c.shape == (0, 3) and f.shape == (0, 3)
        return v, c, f
    assert np.array_equal(f, tf) and np.array_equal(c, tc)
    assert v.tobytes() == tv.astype(np.float32).tobytes()
    assert f.min() >= 0 and f.max() < v.shape[0]
    return v, c, f


# ---- 1. integration against the twins --------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["u8", "f32"])
@pytest.mark.parametrize("K,H,W,seed", CT.SHARED)
def test_integration_and_extraction_against_the_twins(dev, K, H, W, seed, layout):
    sc, pin, vol = scene(K, H, W, seed, layout), CT.shared_pinhole(H, W), TT.VOLUME
    frames = RS.frames_of(sc, dev)
    for thr in (1.5, None):                                                    # a threshold case and none; NaN / inf are planted
        tw64, tw32 = twins(K, H, W, seed, layout, thr)
        volume = fuse(frames, pin, vol, dev, c_conf_threshold=thr)
        out = host(volume)
        TT.check_integration(out, tw64, tw32, sc, vol, f"{K}x{H}x{W} {layout} thr={thr}")
        assert tw64["weight"].max() == K
        v, _, f = check_extraction(volume, out, 1, f"{K}x{H}x{W} {layout} thr={thr}")
        assert v.shape[0] > 500 and f.shape[0] > 500
        if thr == 1.5:
            v2, _, f2 = check_extraction(volume, out, 2, f"{K}x{H}x{W} {layout}")
            assert 0 < v2.shape[0] < v.shape[0] and 0 < f2.shape[0] < f.shape[0]
    # explicit bounds give the same grid and the same bytes
    again = fusion.fuse_tsdf(frames, pin, vol["vs"], bounds=TT.bounds_of(vol), trunc=vol["trunc"], c_conf_threshold=None)
    assert again.origin == volume.origin and same_bytes(host(again), out)


def test_unaligned_keyframes_give_the_same_bytes(dev):
    K, H, W, seed = CT.SHARED[1]
    sc, pin, vol = scene(K, H, W, seed), CT.shared_pinhole(H, W), TT.VOLUME
    frames = RS.frames_of(sc, dev)
    ref = host(fuse(frames, pin, vol, dev))
    for f in frames[::2]:
        for name in ("X_canon", "C"):
            t = getattr(f, name)
            buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
            buf[1:] = t.reshape(-1)
            setattr(f, name, buf[1:].view(t.shape))
            assert getattr(f, name).data_ptr() % 16 != 0
    assert same_bytes(ref, host(fuse(frames, pin, vol, dev)))


@pytest.mark.parametrize("dims", [(2, 2, 2), (2, 3, 70)])
def test_small_volumes(dev, dims):
    K, H, W, seed = CT.SHARED[0]
    sc, pin = scene(K, H, W, seed), CT.shared_pinhole(H, W)
    # around the surface on the optical axis: z = 2.5 lies between the two layers
    vol = TT.volume(dims, origin=[-0.0625 if dims[2] == 2 else -2.1875, -0.0625, 2.4375], vs=2.0 ** -4)
    tw64, tw32 = (TT.integrate(sc, pin, vol, dtype=d) for d in (np.float64, np.float32))
    volume = fuse(RS.frames_of(sc, dev), pin, vol, dev)
    out = host(volume)
    TT.check_integration(out, tw64, tw32, sc, vol, f"dims {dims}")
    assert tw64["weight"].max() >= 2
    check_extraction(volume, out, 1, f"dims {dims}")


def test_a_single_keyframe_and_an_empty_map(dev):
    sc, pin, vol = scene(1, 33, 65, 14), CT.shared_pinhole(33, 65), TT.VOLUME
    tw64, tw32 = (TT.integrate(sc, pin, vol, dtype=d) for d in (np.float64, np.float32))
    volume = fuse(RS.frames_of(sc, dev), pin, vol, dev)
    out = host(volume)
    TT.check_integration(out, tw64, tw32, sc, vol, "K=1")
    assert out[1].max() == 1
    check_extraction(volume, out, 1, "K=1")
    empty = fusion.fuse_tsdf([], pin, vol["vs"], bounds=TT.bounds_of(vol), trunc=vol["trunc"])   # K = 0: the unobserved volume
    t, w, c, m = host(empty)
    assert empty.dims == vol["dims"] and (t == 1).all() and not w.any() and not c.any() and not m.any()
    v, c, f = fusion.extract_surface(empty)
    assert v.shape == (0, 3) and c.shape == (0, 3) and f.shape == (0, 3) and f.dtype == torch.int32
    filled = out_of(vol, dev)
    filled.tsdf.fill_(-3.0)
    assert fusion.fuse_tsdf([], "estimate", vol["vs"], trunc=vol["trunc"], out=filled) is filled and (filled.tsdf == 1).all()


# ---- 2. extraction of an uploaded volume -----------------------------------------------------------------------------
def test_sphere_volume(dev):
    arrays = TT.sphere_volume()
    t, w, c, m = (torch.from_numpy(a).to(dev) for a in arrays)
    volume = fusion.TSDFVolume(t, w, c, tuple(float(v) for v in TT.SPHERE_ORIGIN), TT.SPHERE_VS, 4.0, m)
    v, _, f = check_extraction(volume, arrays, 1, "sphere")
    E, most, least = TT.mesh_topology(f)
    assert (v.shape[0], f.shape[0]) == (1028, 2052) and most == least == 2 and v.shape[0] - E + f.shape[0] == 2
    assert np.abs(np.linalg.norm(v.astype(np.float64) - TT.SPHERE_CENTRE, axis=1) - TT.SPHERE_RADIUS).max() <= np.sqrt(3.0)
    check_extraction(volume, arrays, 2, "sphere")                               # nothing is valid: an empty mesh
    # weights 2 on the lower half: min_weight = 2 keeps the part of the surface whose cells lie entirely in it
    w2 = arrays[1].copy()
    w2[:12] = 2
    half = fusion.TSDFVolume(t, torch.from_numpy(w2).to(dev), c, volume.origin, TT.SPHERE_VS, 4.0, m)
    arrays2 = (arrays[0], w2, arrays[2], arrays[3])
    v1, _, f1 = check_extraction(half, arrays2, 1, "sphere, weights 1 | 2")
    v2, _, f2 = check_extraction(half, arrays2, 2, "sphere, weights 1 | 2")
    assert v1.shape[0] == 1028 and 0 < v2.shape[0] < 1028 and 0 < f2.shape[0] < f1.shape[0]
    assert v2[:, 2].max() < 12 and v2.tobytes() == v1[:v2.shape[0]].tobytes()   # ascending (z, y, x): a prefix
    # colored None: every voxel counts as coloured
    plain = fusion.TSDFVolume(t, w, c, volume.origin, TT.SPHERE_VS, 4.0, None)
    check_extraction(plain, (arrays[0], arrays[1], arrays[2], None), 1, "sphere, colored=None")


# ---- 3. determinism, launches, capture -------------------------------------------------------------------------------
def test_identical_bytes_on_two_calls(dev):
    K, H, W, seed = CT.SHARED[2]
    sc, pin, vol = scene(K, H, W, seed), CT.shared_pinhole(H, W), TT.VOLUME
    frames = RS.frames_of(sc, dev)
    a, b = fuse(frames, pin, vol, dev), fuse(frames, pin, vol, dev)
    assert same_bytes(host(a), host(b)) and a.weight.any()
    ma, mb = mesh_host(fusion.extract_surface(a)), mesh_host(fusion.extract_surface(b))
    assert same_bytes(ma, mb) and ma[2].shape[0] > 0


def captured_nodes(fn):
    """The launches fn(stream) queues, counted as the nodes of a stream capture of one call (captured, never replayed),
    through the HIP runtime the library itself is linked against."""
    hip = ctypes.CDLL(_ffi.LIB_PATH)                                          # dlsym also searches the library's dependencies
    for name in ("hipStreamBeginCapture", "hipStreamEndCapture", "hipGraphGetNodes", "hipGraphDestroy"):
        getattr(hip, name).restype = ctypes.c_int
    hip.hipStreamBeginCapture.argtypes = [ctypes.c_void_p, ctypes.c_int]
    hip.hipStreamEndCapture.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    hip.hipGraphDestroy.argtypes = [ctypes.c_void_p]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph, nodes = ctypes.c_void_p(), ctypes.c_size_t(0)
    assert hip.hipStreamBeginCapture(side.cuda_stream, 2) == 0                # hipStreamCaptureModeRelaxed
    rc = fn(side.cuda_stream)
    assert hip.hipStreamEndCapture(side.cuda_stream, ctypes.byref(graph)) == 0 and rc == 0
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(nodes)) == 0
    assert hip.hipGraphDestroy(graph) == 0
    return nodes.value


@pytest.mark.parametrize("K", [1, 5])
def test_launch_counts_are_the_documented_constants(dev, K):
    L = _ffi.lib()
    H, W = 33, 65
    sc, pin, vol = scene(K, H, W, 20 + K), CT.shared_pinhole(H, W), TT.VOLUME
    frames = RS.frames_of(sc, dev)
    m = render.map_tables(frames)
    want = fuse(frames, pin, vol, dev)
    out = out_of(vol, dev)
    ws = torch.empty(fusion.workspace_bytes(K, H * W), dtype=torch.uint8, device=dev)
    dz, dy, dx = vol["dims"]
    o = [float(v) for v in vol["origin"]]
    integrate = lambda stream: L.m3_tsdf_integrate(
        _ffi.ptr(m.table[0]), _ffi.ptr(m.table[1]), _ffi.ptr(m.table[2]), _ffi.ptr(m.poses), _ffi.ptr(m.nk), m.k, H, W, 1, 1.5,
        m.layout, *pin, 1e-3, *o, vol["vs"], vol["trunc"], dx, dy, dz, _ffi.ptr(ws), ws.numel(), _ffi.ptr(out.tsdf),
        _ffi.ptr(out.weight), _ffi.ptr(out.color), _ffi.ptr(out.colored), stream)
    nodes = captured_nodes(integrate)
    print(f"K={K}: {nodes} graph nodes for one integration")
    assert nodes == L.m3_tsdf_integrate_launches() == 3
    assert integrate(_ffi.stream_ptr()) == 0                                   # the same arguments, run: the eager result
    assert same_bytes(host(out), host(want))
    # extraction: count and scatter are captured apart (the host reads V and F between them)
    ews = torch.empty(L.m3_tsdf_extract_ws_bytes(dx, dy, dz), dtype=torch.uint8, device=dev)
    v, c, f = fusion.extract_surface(want)
    vo, co, fo = torch.empty_like(v), torch.empty_like(c), torch.empty_like(f)
    count = lambda stream: L.m3_tsdf_extract_count(_ffi.ptr(out.tsdf), _ffi.ptr(out.weight), dx, dy, dz, 1, _ffi.ptr(ews),
                                                   ews.numel(), stream)
    scatter = lambda stream: L.m3_tsdf_extract_scatter(
        _ffi.ptr(out.tsdf), _ffi.ptr(out.weight), _ffi.ptr(out.color), _ffi.ptr(out.colored), *o, vol["vs"], dx, dy, dz, 1,
        _ffi.ptr(ews), ews.numel(), v.shape[0], f.shape[0], _ffi.ptr(vo), _ffi.ptr(co), _ffi.ptr(fo), stream)
    n_count, n_scatter = captured_nodes(count), captured_nodes(scatter)
    print(f"K={K}: {n_count} + {n_scatter} graph nodes for one extraction")
    assert n_count + n_scatter == L.m3_tsdf_extract_launches() == 5 and n_scatter == 2
    assert count(_ffi.stream_ptr()) == 0
    assert ews[:8].view(torch.int32).tolist() == [v.shape[0], f.shape[0] // 2]
    assert scatter(_ffi.stream_ptr()) == 0
    assert same_bytes(mesh_host((vo, co, fo)), mesh_host((v, c, f))) and f.shape[0] > 0


def test_graph_replay_reads_the_poses_on_the_device(dev):
    K, H, W, seed = CT.SHARED[0]
    sc, pin, vol = scene(K, H, W, seed), CT.shared_pinhole(H, W), TT.VOLUME
    frames = RS.frames_of(sc, dev)
    new_pose = sc["T"][1].copy()
    new_pose[:3] += np.float32([0.05, -0.02, 0.08])
    new_pose[7] *= np.float32(1.02)
    want_a = host(fuse(frames, pin, vol, dev))
    out = out_of(vol, dev)
    ws = torch.empty(fusion.workspace_bytes(K, H * W), dtype=torch.uint8, device=dev)
    tables = render.map_tables(frames)                                       # host-to-device copies stay outside the capture
    kw = dict(bounds=TT.bounds_of(vol), trunc=vol["trunc"], out=out, workspace=ws)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                            # warm-up outside the capture
        fusion.fuse_tsdf(tables, pin, vol["vs"], **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                             # one stream: a serial chain of launches
        fusion.fuse_tsdf(tables, pin, vol["vs"], **kw)
    for t in (out.tsdf, out.weight, out.color, out.colored):
        t.zero_()
    graph.replay()
    assert same_bytes(host(out), want_a)
    frames[1].T_WC.copy_(torch.from_numpy(new_pose).to(dev).reshape(1, 8))   # in place: the graph reads this tensor
    graph.replay()
    got_b = host(out)
    want_b = host(fuse(frames, pin, vol, dev))                                # eager, on the new pose
    assert same_bytes(got_b, want_b) and not same_bytes(want_a, want_b)


# ---- 4. consistency views --------------------------------------------------------------------------------------------
def test_consistent_keyframes_fuse_with_fewer_observed_voxels(dev):
    K, H, W, seed = CT.SHARED[1]
    sc, pin, vol = scene(K, H, W, seed, "f32"), CT.shared_pinhole(H, W), TT.VOLUME
    frames = RS.frames_of(sc, dev, shape=(H, W))
    views = consistency.consistent_keyframes(frames, pin, neighbours=None)
    a, b = fuse(frames, pin, vol, dev), fuse(views, pin, vol, dev)
    na, nb = int((a.weight > 0).sum()), int((b.weight > 0).sum())
    print(f"{na} observed voxels, {nb} from the consistent views")
    assert 0 < nb < na and bool((b.weight <= a.weight).all())
    v, c, f = fusion.extract_surface(b)
    assert f.shape[0] > 0 and int(f.max()) < v.shape[0]
    # the default volume: the box of the exported points
    auto = fusion.fuse_tsdf(views, pin, vol["vs"])
    lo, hi = fusion.map_bounds(views)
    assert auto.dims == fusion.volume_grid((lo, hi), vol["vs"])[1] and bool((auto.weight > 0).any())
