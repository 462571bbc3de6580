"""GPU: connected components and the fragment filter (csrc/mesh_components.hip through components.mesh_components /
filter_components) against the numpy twin (tests/components_twin.py).  Every output is compared exactly - labels, counts,
info, vertices as bytes, colours, faces, both row indices - and every case runs twice for identical bytes.  The meshes
are the smallest at which the kernels can go wrong: deep and colliding trees, ties, rows no face names, tiles that are
not full, and tile counts beyond one round of the scan."""
import ctypes

import numpy as np
import pytest
import torch

import components_twin as CC
import consistency_twin as CT
import render_scenes as RS
import tsdf_twin as TT
from mast3r_slam import _ffi, components, fusion, render

pytestmark = pytest.mark.gpu


def upload(mesh, dev):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in mesh)


def same_bytes(a, b):
    """Tensor tuples with the same dtypes, shapes and bytes (vertices hold a NaN: equality of values would not do)."""
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
                                    for x, y in zip(a, b))


def check_labels(mesh, dev, label=""):
    """mesh_components against the twin, twice."""
    V = mesh[0].shape[0]
    want_lab, want_of, want_info, invalid = CC.components(mesh[2], V)
    assert invalid == 0
    faces = upload(mesh, dev)[2]
    for _ in range(2):
        lab, of, info = components.mesh_components(faces, V)
        assert lab.dtype == torch.int32 and of.dtype == torch.int32 and lab.is_cuda and lab.shape == (V,) and of.shape == (V,)
        assert np.array_equal(lab.cpu().numpy(), want_lab) and np.array_equal(of.cpu().numpy(), want_of)
        assert tuple(info) == tuple(want_info), (label, info, want_info)
    print(f"{label}: V={V} F={mesh[2].shape[0]} {want_info}")
    return want_lab, want_of, want_info


def check_filter(mesh, dev, label="", **kw):
    """filter_components against the twin, twice with the row indices and once without.  Returns the twin's result."""
    want = CC.filter_mesh(*mesh, **kw)
    t = upload(mesh, dev)
    for _ in range(2):
        got = components.filter_components(*t, return_index=True, **kw)
        assert [g.dtype for g in got] == [torch.float32, torch.uint8, torch.int32, torch.int64, torch.int64]
        assert all(g.is_cuda for g in got) and got[0].shape[1:] == (3,) and got[1].shape[1:] == (3,) and got[2].shape[1:] == (3,)
        host = [g.cpu().numpy() for g in got]
        assert [h.shape for h in host] == [w.shape for w in want], (label, kw)
        assert host[0].tobytes() == want[0].tobytes() and np.array_equal(host[1], want[1])
        assert np.array_equal(host[2], want[2]) and np.array_equal(host[3], want[3]) and np.array_equal(host[4], want[4])
    plain = components.filter_components(t, **kw)                               # the tuple, whole
    assert len(plain) == 3 and same_bytes(plain, got[:3])
    print(f"{label} {kw}: {want[0].shape[0]} of {mesh[0].shape[0]} vertices, {want[2].shape[0]} of {mesh[2].shape[0]} faces")
    return want


# ---- strips: deep trees, colliding hooks -----------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["shuffled", "descending"])
def test_one_strip_is_one_component(dev, order):
    mesh = CC.strip(5000, order, seed=21)
    lab, of, info = check_labels(mesh, dev, order)
    assert info == (1, 5000, 0) and not lab.any() and (of == 5000).all()       # the label is the smallest row
    v, c, f, rows_v, rows_f = check_filter(mesh, dev, order, largest_only=True)
    assert v.shape[0] == 5002 and np.array_equal(f, mesh[2])                   # everything is kept, as it came


# ---- islands: ties and thresholds ------------------------------------------------------------------------------------
def test_many_islands(dev):
    mesh = CC.islands()
    lab, of, info = check_labels(mesh, dev, "islands")
    sizes = sorted(set(CC.ISLAND_SIZES) | {1})
    assert info.components == 3000 + len(CC.ISLAND_SIZES) and info.largest == 40 and sorted(set(of.tolist())) == sizes
    roots = np.flatnonzero((lab == np.arange(lab.shape[0])) & (of == 40))
    assert roots.shape[0] == 3 and info.winner == roots.min()                   # the tie goes to the smaller label
    for n in sizes:                                                            # each size as the bound, and one above it
        for bound in (n, n + 1):
            want = check_filter(mesh, dev, "islands", min_faces=bound)
            assert want[2].shape[0] == sum(s for s in (1,) * 3000 + CC.ISLAND_SIZES if s >= bound)
    want = check_filter(mesh, dev, "islands", largest_only=True)
    assert want[2].shape[0] == 40 and (lab[want[3]] == roots.min()).all()
    # 0.125 * 40 is exactly 5 faces; the next fp32 above 0.125 asks for more than 5
    assert check_filter(mesh, dev, "islands", min_fraction=0.125)[2].shape[0] == sum(s for s in CC.ISLAND_SIZES if s >= 5)
    above = float(np.nextafter(np.float32(0.125), np.float32(1)))
    assert check_filter(mesh, dev, "islands", min_fraction=above)[2].shape[0] == sum(s for s in CC.ISLAND_SIZES if s > 5)
    assert check_filter(mesh, dev, "islands", min_fraction=0.3)[2].shape[0] == 13 + 20 + 39 + 120    # 0.3f * 40 > 12
    assert check_filter(mesh, dev, "islands", min_fraction=1.0, min_faces=7)[2].shape[0] == 120
    assert check_filter(mesh, dev, "islands", min_fraction=0.5, largest_only=True)[2].shape[0] == 40


# ---- connectivity is by row ------------------------------------------------------------------------------------------
def test_fans_and_twin_rows(dev):
    joined, apart = CC.fans(False), CC.fans(True)
    assert check_labels(joined, dev, "fans, one shared row")[2] == (1, 14, 0)
    lab, of, info = check_labels(apart, dev, "fans, a twin row")
    assert info == (2, 7, 0) and lab[-1] == 9 and apart[0][8].tobytes() == apart[0][-1].tobytes()
    assert check_filter(joined, dev, "fans", largest_only=True)[2].shape[0] == 14
    assert check_filter(apart, dev, "fans", largest_only=True)[2].shape[0] == 7


def test_unreferenced_vertices(dev):
    base = CC.islands(300, (2, 9, 9))
    V = base[0].shape[0]
    mesh = CC.with_unreferenced(base, [0, 0, V // 2, V // 2 + 1, V, V, V])      # at the start, in the middle, at the end
    lab, of, info = check_labels(mesh, dev, "unreferenced")
    loose = np.setdiff1d(np.arange(mesh[0].shape[0]), mesh[2].reshape(-1))
    assert loose.shape[0] == 7 and loose[0] == 0 and loose[-1] == mesh[0].shape[0] - 1
    assert np.array_equal(lab[loose], loose) and not of[loose].any()            # its own label, no face
    for kw in (dict(), dict(min_faces=2), dict(largest_only=True), dict(min_fraction=0.2)):
        want = check_filter(mesh, dev, "unreferenced", **kw)
        assert not np.isin(want[3], loose).any()                                # dropped by every filter
        assert np.array_equal(want[3][want[2]], mesh[2][want[4]])               # the remap is right around them
    # the default filter drops nothing else: the result is the mesh without those rows
    assert check_filter(mesh, dev, "unreferenced")[0].tobytes() == base[0].tobytes()


def test_degenerate_and_invalid_faces(dev):
    f = np.array([[0, 0, 1], [2, 3, 3], [1, 2, 2], [4, 5, 6], [6, 6, 6], [7, 8, 7]], dtype=np.int32)
    mesh = CC.arrays(10, 3) + (f,)
    lab, of, info = check_labels(mesh, dev, "degenerate")                       # a row named twice connects and counts
    assert lab.tolist() == [0, 0, 0, 0, 4, 4, 4, 7, 7, 9] and of.tolist() == [3] * 4 + [2] * 3 + [1, 1, 0] and info == (3, 3, 0)
    assert check_filter(mesh, dev, "degenerate", min_faces=2)[2].shape[0] == 5
    v, c, faces = upload(mesh, dev)
    for row in (10, -1):                                                        # == V, and below 0
        for at in (0, 5):
            bad = faces.clone()
            bad[at, 1] = row
            with pytest.raises(ValueError, match="outside"):
                components.mesh_components(bad, 10)
            with pytest.raises(ValueError, match="outside"):
                components.filter_components(v, c, bad)


# ---- shapes ----------------------------------------------------------------------------------------------------------
def test_shape_edges(dev, monkeypatch):
    one = CC.arrays(3, 1) + (np.array([[2, 0, 1]], dtype=np.int32),)
    assert check_labels(one, dev, "F=1")[2] == (1, 1, 0)
    assert check_filter(one, dev, "F=1")[2].tolist() == [[2, 0, 1]]
    none = CC.arrays(5, 2) + (np.zeros((0, 3), dtype=np.int32),)
    lab, of, info = check_labels(none, dev, "F=0")
    assert lab.tolist() == [0, 1, 2, 3, 4] and not of.any() and info == (0, 0, -1)
    empty = CC.arrays(0, 2) + (np.zeros((0, 3), dtype=np.int32),)
    assert check_labels(empty, dev, "V=0")[2] == (0, 0, -1)
    for mesh in (none, empty):
        out = check_filter(mesh, dev, "empty")
        assert [o.shape for o in out] == [(0, 3), (0, 3), (0, 3), (0,), (0,)]
    # V and F that are no multiple of the 256-row tile, over several tiles
    odd = CC.islands(700, (3, 30))
    assert odd[0].shape[0] % 256 and odd[2].shape[0] % 256 and odd[2].shape[0] > 512
    check_labels(odd, dev, "odd")
    check_filter(odd, dev, "odd", min_faces=3)
    # a filter that keeps nothing: the empty mesh, and no scatter is launched
    calls = {}
    monkeypatch.setattr(_ffi, "PROFILE", calls)
    monkeypatch.setattr(_ffi, "PROFILE_NAMES", ("m3_mesh_components_label", "m3_mesh_components_count", "m3_mesh_components_scatter"))
    out = components.filter_components(upload(odd, dev), min_faces=31, return_index=True)
    assert sorted(calls) == ["m3_mesh_components_count", "m3_mesh_components_label"]
    assert [tuple(o.shape) for o in out] == [(0, 3), (0, 3), (0, 3), (0,), (0,)]
    assert [o.dtype for o in out] == [torch.float32, torch.uint8, torch.int32, torch.int64, torch.int64] and out[0].is_cuda
    components.filter_components(upload(odd, dev), min_faces=30)
    assert "m3_mesh_components_scatter" in calls


def test_tiles_beyond_one_round_of_the_scan(dev):
    """4101 vertex tiles: the scan of the kept-vertex counts takes a second round of 4096, and kept vertices lie beyond it."""
    V = 4100 * 256 + 77
    mesh = CC.scattered_triangles(V, 30000, seed=3)
    assert (V + 255) // 256 > 4096
    lab, of, info = check_labels(mesh, dev, "tall")
    assert info == (30001, 2, V - 4)
    want = check_filter(mesh, dev, "tall")
    assert want[0].shape[0] == 90004 and int((want[3] >= 4096 * 256).sum()) > 4
    want = check_filter(mesh, dev, "tall", min_faces=2)                         # only the strip in the last rows
    assert want[3].tolist() == [V - 4, V - 3, V - 2, V - 1] and want[2].shape[0] == 2


def test_workspace_argument(dev):
    mesh = CC.islands(100, (4, 4))
    t = upload(mesh, dev)
    need = components.workspace_bytes(mesh[0].shape[0], mesh[2].shape[0])
    ws = torch.empty(need + 64, dtype=torch.uint8, device=dev)
    a = components.filter_components(*t, min_faces=4, workspace=ws)
    b = components.filter_components(*t, min_faces=4)
    assert same_bytes(a, b) and a[2].shape[0] == 8
    assert same_bytes(components.mesh_components(t[2], t[0].shape[0], workspace=ws)[:2],
                      components.mesh_components(t[2], t[0].shape[0])[:2])
    for bad in (ws[:need - 16], ws[8:], ws.to(torch.int8)):
        with pytest.raises((ValueError, TypeError)):
            components.filter_components(*t, workspace=bad)


# ---- a fused mesh with a genuine fragment ----------------------------------------------------------------------------
def test_fused_mesh_fragment(dev):
    K, H, W, seed = CT.SHARED[0]
    sc, pin, vol = CT.shared_scene(K, H, W, seed), CT.shared_pinhole(H, W), TT.VOLUME
    frames = RS.frames_of(sc, dev)
    volume = fusion.fuse_tsdf(frames, pin, vol["vs"], bounds=TT.bounds_of(vol), trunc=vol["trunc"])
    before = fusion.extract_surface(volume)
    # a blob off the surface: 5^3 voxels of unobserved space get one observation each, free but for the one in the middle
    unseen = volume.weight.cpu().numpy() == 0
    room = np.argwhere(np.lib.stride_tricks.sliding_window_view(unseen, (7, 7, 7)).all(axis=(3, 4, 5)))
    assert room.shape[0] > 0
    z, y, x = (int(i) + 3 for i in room[0])
    volume.weight[z - 2:z + 3, y - 2:y + 3, x - 2:x + 3] = 1
    volume.tsdf[z - 2:z + 3, y - 2:y + 3, x - 2:x + 3] = 1.0
    volume.tsdf[z, y, x] = -0.5
    mesh_dev = fusion.extract_surface(volume)
    mesh = tuple(t.cpu().numpy() for t in mesh_dev)
    assert mesh[0].shape[0] == before[0].shape[0] + 8 and mesh[2].shape[0] == before[2].shape[0] + 12   # a cube around the voxel
    lab, of, info = check_labels(mesh, dev, "fused")
    assert info.components >= 2 and 12 in of.tolist() and info.largest > 100
    want = check_filter(mesh, dev, "fused", largest_only=True)
    assert want[2].shape[0] == info.largest
    check_filter(mesh, dev, "fused", min_faces=13)
    clean = components.filter_components(mesh_dev, largest_only=True)
    again = components.mesh_components(clean[2], clean[0].shape[0])
    assert again[2] == (1, info.largest, 0) and not again[0].any()              # exactly one component when labelled again
    rgb, depth = render.render_mesh(clean, frames[0].T_WC, pin, (H, W))
    assert rgb.shape == (H, W, 3) and bool(torch.isfinite(depth).any())


# ---- launches and capture --------------------------------------------------------------------------------------------
def captured_nodes(fn):
    """The launches fn(stream) queues, counted as the nodes of a stream capture of one call (captured, never replayed),
    through the HIP runtime the library itself is linked against."""
    hip = ctypes.CDLL(_ffi.LIB_PATH)
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


@pytest.mark.parametrize("which", ["islands", "strip"])
def test_launch_counts_are_the_documented_constants(dev, which):
    L = _ffi.lib()
    mesh = CC.islands(200, (5, 6)) if which == "islands" else CC.strip(900, "shuffled", 2)
    v, c, f = upload(mesh, dev)
    V, F = v.shape[0], f.shape[0]
    want = components.filter_components(v, c, f, min_faces=2, return_index=True)
    ws = torch.empty(components.workspace_bytes(V, F), dtype=torch.uint8, device=dev)
    lab, of = torch.empty(V, dtype=torch.int32, device=dev), torch.empty(V, dtype=torch.int32, device=dev)
    out = [torch.empty_like(t) for t in want]
    label = lambda st: L.m3_mesh_components_label(_ffi.ptr(f), V, F, _ffi.ptr(ws), ws.numel(), _ffi.ptr(lab), _ffi.ptr(of), st)
    count = lambda st: L.m3_mesh_components_count(_ffi.ptr(ws), V, F, _ffi.ptr(f), 2, 0.0, 0, st)
    scatter = lambda st: L.m3_mesh_components_scatter(_ffi.ptr(v), _ffi.ptr(c), _ffi.ptr(f), V, F, _ffi.ptr(ws), out[0].shape[0],
                                                      out[2].shape[0], *[_ffi.ptr(o) for o in out], st)
    n = [captured_nodes(fn) for fn in (label, count, scatter)]
    print(f"{which}: {n} graph nodes for label, count, scatter")
    assert n == [6, 3, 2] and sum(n) == L.m3_mesh_components_launches() == 11
    st = _ffi.stream_ptr()
    assert label(st) == 0 and count(st) == 0
    assert ws[:8].view(torch.int32).tolist() == [out[0].shape[0], out[2].shape[0]]
    assert scatter(st) == 0
    assert same_bytes(out, want) and out[2].shape[0] > 0


def test_graph_replay_gives_the_eager_bytes(dev):
    mesh = CC.islands(500, (7, 7, 3))
    v, c, f = upload(mesh, dev)
    V, F = v.shape[0], f.shape[0]
    ws = torch.empty(components.workspace_bytes(V, F), dtype=torch.uint8, device=dev)
    lab, of = torch.empty(V, dtype=torch.int32, device=dev), torch.empty(V, dtype=torch.int32, device=dev)

    def queue():
        st = _ffi.stream_ptr()
        _ffi.call("m3_mesh_components_label", _ffi.ptr(f), V, F, _ffi.ptr(ws), ws.numel(), _ffi.ptr(lab), _ffi.ptr(of), st)
        _ffi.call("m3_mesh_components_count", _ffi.ptr(ws), V, F, _ffi.ptr(f), 3, 0.0, 0, st)

    queue()
    eager = (lab.clone(), of.clone(), ws[:32].clone())
    want_lab, want_of, info, _ = CC.components(mesh[2], V)
    assert np.array_equal(eager[0].cpu().numpy(), want_lab) and eager[2].view(torch.int32).tolist()[:2] == [23, 17]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                              # warm-up outside the capture
        queue()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                               # one stream: a serial chain of launches
        queue()
    for t in (lab, of, ws):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(lab, eager[0]) and torch.equal(of, eager[1]) and torch.equal(ws[:32], eager[2])
