"""GPU: mesh simplification by vertex clustering (csrc/mesh_simplify.hip through simplify.simplify_mesh) against the numpy
twin (tests/simplify_twin.py).  Every output is compared as bytes - vertices, colours, faces, cluster_of, face_rows -
and every case runs twice for identical bytes.  The meshes are the smallest at which the kernels can go wrong: clusters
of one and of hundreds, several compaction tiles that are not full, vertices on cell boundaries, out-of-range vertices,
repeated faces of either winding, vertices no face names, and nothing at all."""
import ctypes

import numpy as np
import pytest
import torch

import simplify_twin as ST
from mast3r_slam import _ffi, simplify

pytestmark = pytest.mark.gpu
VOXEL = 2.5 * ST.SPACING
DTYPES = [torch.float32, torch.uint8, torch.int32, torch.int64, torch.int64]


def upload(mesh, dev):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in mesh[:3])


def host(out):
    return [o.cpu().numpy() for o in out]


def same_bytes(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.fixture(scope="module")
def grids():
    """The shared scenes and the twin's result on them, computed once: name -> (mesh, voxel, twin)."""
    small, large = ST.grid_mesh(), ST.grid_mesh(70, 70)
    cases = {"grid": (small, VOXEL), "tiles": (large, VOXEL), "coarse": (large, 100 * ST.SPACING), "fine": (small, 0.1 * ST.SPACING)}
    return {k: (m, vox, ST.simplify(*m, vox)) for k, (m, vox) in cases.items()}


def check(mesh, voxel, dev, want=None, label=""):
    """simplify_mesh against the twin, twice with the indices and once without, whole.  Returns the twin's result."""
    want = want or ST.simplify(*mesh, voxel)
    t = upload(mesh, dev)
    for _ in range(2):
        got = simplify.simplify_mesh(*t, voxel_size=voxel, return_index=True)
        assert [g.dtype for g in got] == DTYPES and all(g.is_cuda for g in got)
        got = host(got)
        assert [g.shape for g in got] == [w.shape for w in want[:5]], (label, [g.shape for g in got])
        for name, g, w in zip(("vertices", "colors", "faces", "cluster_of", "face_rows"), got, want[:5]):
            assert g.tobytes() == w.tobytes(), (label, name, int((g != w).sum()))
    plain = simplify.simplify_mesh(t, voxel_size=voxel)                          # the tuple, whole
    assert len(plain) == 3 and same_bytes(host(plain), got[:3])
    info = simplify.simplify_counts(t, voxel_size=voxel)
    assert info == (want[0].shape[0], want[2].shape[0], want[5]["out_of_range"])
    n = want[5]["sizes"]
    print(f"{label}: V {mesh[0].shape[0]} -> {want[0].shape[0]}, F {mesh[2].shape[0]} -> {want[2].shape[0]}, largest cluster "
          f"{int(n.max()) if n.size else 0}, out of range {want[5]['out_of_range']}")
    return want


# ---- the jittered grid -----------------------------------------------------------------------------------------------
def test_grid_at_a_voxel_of_two_and_a_half_spacings(dev, grids):
    mesh, voxel, want = grids["grid"]
    check(mesh, voxel, dev, want, "grid")
    n = want[5]["sizes"]
    assert (n == 1).any() and n.max() >= 4 and want[5]["collapsed"] and want[5]["repeats"]


def test_grid_across_several_tiles(dev, grids):
    mesh, voxel, want = grids["tiles"]
    assert mesh[0].shape[0] == 4900 and want[0].shape[0] > 1024 and want[2].shape[0] > 2048 and want[5]["repeats"]
    leaders = np.unique(want[3], return_index=True)[1]
    assert leaders.max() >= 1024 and want[4].max() >= 2048                      # leaders and kept faces beyond the first tiles
    check(mesh, voxel, dev, want, "tiles")


def test_coarse_voxel_with_contended_sums(dev, grids):
    mesh, voxel, want = grids["coarse"]
    n = want[5]["sizes"]
    assert want[0].shape[0] <= 8 and n.min() >= 100                              # a handful of clusters, hundreds of members each
    check(mesh, voxel, dev, want, "coarse")


def test_fine_voxel_returns_the_arrays(dev, grids):
    mesh, voxel, want = grids["fine"]
    check(mesh, voxel, dev, want, "fine")
    v, c, f = upload(mesh, dev)
    out = simplify.simplify_mesh(v, c, f, voxel_size=voxel)
    assert torch.equal(out[0].view(torch.int32), v.view(torch.int32)) and torch.equal(out[1], c)
    assert np.array_equal(out[2].cpu().numpy(), ST.rotate_min_first(mesh[2]))


# ---- edges of the rule -----------------------------------------------------------------------------------------------
def test_cell_boundaries_and_negative_coordinates(dev):
    mesh = ST.boundary_mesh()
    want = check(mesh, 0.25, dev, label="boundaries")
    on = 19 * 19
    cell = np.round(mesh[0][:on, :2] / 0.25).astype(np.int64)
    assert (mesh[0][:on, :2] == cell * np.float32(0.25)).all() and cell.min() == -9 and cell.max() == 9
    # a vertex at k * voxel lies in cell k: its cluster's output stays inside [k, k + 1) * voxel
    out = want[0][want[3][:on]]
    assert (out[:, :2] >= mesh[0][:on, :2]).all() and (out[:, :2] < mesh[0][:on, :2] + np.float32(0.25)).all()
    assert want[5]["sizes"].max() == 2


def test_out_of_range_vertices(dev):
    base = ST.boundary_mesh()
    mesh = ST.with_out_of_range(base)
    want = check(mesh, 0.25, dev, label="out of range")
    clean = ST.simplify(*base, 0.25)
    V = base[0].shape[0]
    assert want[5]["out_of_range"] == 3 and want[3][[5, V + 1, V + 2]].tolist() == [-1, -1, -1]
    assert want[0].tobytes() == clean[0].tobytes() and want[1].tobytes() == clean[1].tobytes()      # dropped and counted
    assert want[5]["out_faces"] >= 3 and np.array_equal(want[2], clean[2])       # the faces that name them are gone
    assert not np.isin(want[4], np.arange(mesh[2].shape[0] - 3, mesh[2].shape[0])).any()


@pytest.mark.parametrize("opposite", [False, True])
def test_two_faces_over_the_same_clusters(dev, opposite):
    want = check(ST.winding_pair(opposite), 1.0, dev, label=f"opposite={opposite}")
    assert want[2].tolist() == ([[0, 1, 2], [0, 2, 1]] if opposite else [[0, 1, 2]])
    assert want[4].tolist() == ([0, 1] if opposite else [0])                    # the smaller row is kept


def test_one_cell_one_vertex_and_unnamed_vertices(dev):
    v, c, _ = ST.grid_mesh(5, 5)
    none = np.zeros((0, 3), dtype=np.int32)
    want = check((v, c, none), 1.0, dev, label="one cell")                      # everything in one cell... of each octant
    assert want[0].shape[0] <= 8
    v1 = np.abs(v) + np.float32(0.001)
    want = check((v1, c, none), 1.0, dev, label="one cell")
    assert want[0].shape[0] == 1 and want[5]["sizes"].tolist() == [25] and want[2].shape == (0, 3)
    want = check((v1[:1], c[:1], none), 1.0, dev, label="one vertex")
    assert want[0].tobytes() == v1[:1].tobytes()
    # vertices that no face names: every cluster is output
    mesh = ST.grid_mesh()
    few = mesh[2][:40]
    want = check((mesh[0], mesh[1], few), VOXEL, dev, label="unnamed")
    assert want[0].shape[0] == 318 and np.unique(want[2]).shape[0] < 318


def test_empty_mesh_and_bad_face_row(dev):
    e = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.int32))
    out = simplify.simplify_mesh(upload(e, dev), voxel_size=0.5, return_index=True)
    assert [tuple(o.shape) for o in out] == [(0, 3), (0, 3), (0, 3), (0,), (0,)] and [o.dtype for o in out] == DTYPES
    assert all(o.is_cuda for o in out) and len(simplify.simplify_mesh(*upload(e, dev), voxel_size=0.5)) == 3
    assert simplify.simplify_counts(upload(e, dev), voxel_size=0.5) == (0, 0, 0)
    # every vertex out of range: no cluster, no face, cluster_of all -1
    v = np.full((4, 3), np.nan, dtype=np.float32)
    want = check((v, np.zeros((4, 3), np.uint8), np.array([[0, 1, 2]], dtype=np.int32)), 0.5, dev, label="all out of range")
    assert want[0].shape[0] == 0 and want[3].tolist() == [-1] * 4
    v, c, f = upload(ST.winding_pair(False), dev)
    for row in (6, -1):                                                         # == V, and below 0
        bad = f.clone()
        bad[1, 2] = row
        with pytest.raises(ValueError, match="outside"):
            simplify.simplify_mesh(v, c, bad, voxel_size=1.0)
        with pytest.raises(ValueError, match="outside"):
            simplify.simplify_counts(v, c, bad, voxel_size=1.0)


# ---- order independence and repeatability ----------------------------------------------------------------------------
def test_order_independence(dev, grids):
    mesh, voxel, want = grids["tiles"]
    rng = np.random.default_rng(9)
    pf = rng.permutation(mesh[2].shape[0])
    got = host(simplify.simplify_mesh(*upload((mesh[0], mesh[1], mesh[2][pf]), dev), voxel_size=voxel, return_index=True))
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and np.array_equal(got[3], want[3])
    assert got[2].shape == want[2].shape and {tuple(t) for t in got[2].tolist()} == {tuple(t) for t in want[2].tolist()}
    pv = rng.permutation(mesh[0].shape[0])                                      # new row i holds old row pv[i]
    where = np.empty_like(pv)
    where[pv] = np.arange(pv.shape[0])
    got = host(simplify.simplify_mesh(*upload((mesh[0][pv], mesh[1][pv], where[mesh[2]].astype(np.int32)), dev), voxel_size=voxel))
    rows = lambda v, c: sorted(zip(v.view(np.uint32).tolist(), c.tolist()))
    assert rows(got[0], got[1]) == rows(want[0], want[1]) and got[2].shape == want[2].shape


def test_repeatability_and_a_used_workspace(dev, grids):
    mesh, voxel, want = grids["grid"]
    large = grids["tiles"][0]
    t, big = upload(mesh, dev), upload(large, dev)
    fresh = host(simplify.simplify_mesh(*t, voxel_size=voxel, return_index=True))
    assert same_bytes(fresh, host(simplify.simplify_mesh(*t, voxel_size=voxel, return_index=True)))
    ws = torch.empty(simplify.workspace_bytes(large[0].shape[0], large[2].shape[0]) + 64, dtype=torch.uint8, device=dev)
    simplify.simplify_mesh(*big, voxel_size=100 * ST.SPACING, workspace=ws)     # a different, larger mesh just before
    used = host(simplify.simplify_mesh(*t, voxel_size=voxel, return_index=True, workspace=ws))
    assert same_bytes(used, fresh) and same_bytes(fresh, list(want[:5]))
    ws.fill_(0xa5)                                                              # and whatever else it held
    assert same_bytes(host(simplify.simplify_mesh(*t, voxel_size=voxel, return_index=True, workspace=ws)), fresh)
    need = simplify.workspace_bytes(mesh[0].shape[0], mesh[2].shape[0])
    for bad in (ws[:need - 16], ws[8:], ws.to(torch.int8)):
        with pytest.raises((ValueError, TypeError)):
            simplify.simplify_mesh(*t, voxel_size=voxel, workspace=bad)


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


def raw_calls(t, voxel, ws, out):
    """count(stream) and scatter(stream) of the C entry points on the device mesh t, writing to the tensors `out`."""
    L = _ffi.lib()
    v, c, f = t
    V, F = v.shape[0], f.shape[0]
    count = lambda st: L.m3_mesh_simplify_count(_ffi.ptr(v), _ffi.ptr(c), _ffi.ptr(f), V, F, voxel, _ffi.ptr(ws), ws.numel(), st)
    scatter = lambda st: L.m3_mesh_simplify_scatter(_ffi.ptr(v), _ffi.ptr(c), _ffi.ptr(f), V, F, _ffi.ptr(ws), ws.numel(),
                                                    out[0].shape[0], out[2].shape[0], *[_ffi.ptr(o) for o in out], st)
    return count, scatter


@pytest.mark.parametrize("which", ["small", "tiles"])
def test_launch_counts_are_the_documented_constants(dev, grids, which):
    mesh, voxel, _ = grids["tiles"] if which == "tiles" else (ST.winding_pair(False), 1.0, None)
    t = upload(mesh, dev)
    want = simplify.simplify_mesh(*t, voxel_size=voxel, return_index=True)
    ws = torch.empty(simplify.workspace_bytes(t[0].shape[0], t[2].shape[0]), dtype=torch.uint8, device=dev)
    out = [torch.empty_like(w) for w in want]
    count, scatter = raw_calls(t, voxel, ws, out)
    n = [captured_nodes(fn) for fn in (count, scatter)]
    print(f"{which}: {n} graph nodes for count, scatter")
    assert n == [6, 2] and sum(n) == _ffi.lib().m3_mesh_simplify_launches() == 8
    st = _ffi.stream_ptr()
    assert count(st) == 0
    assert ws[:16].view(torch.int32).tolist() == [out[0].shape[0], out[2].shape[0], 0, 0]
    assert scatter(st) == 0
    assert same_bytes(host(out), host(want)) and out[2].shape[0] > 0


def test_graph_replay_on_a_mesh_changed_in_place(dev, grids):
    mesh, voxel, _ = grids["grid"]
    other = ST.grid_mesh(seed=6)                                                # the same sizes, other content
    assert other[0].shape == mesh[0].shape and other[2].shape == mesh[2].shape
    t = tuple(x.clone() for x in upload(mesh, dev))
    ws = torch.empty(simplify.workspace_bytes(t[0].shape[0], t[2].shape[0]), dtype=torch.uint8, device=dev)
    L = _ffi.lib()

    def queue():
        _ffi.call("m3_mesh_simplify_count", _ffi.ptr(t[0]), _ffi.ptr(t[1]), _ffi.ptr(t[2]), t[0].shape[0], t[2].shape[0], voxel,
                  _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr())

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                              # warm-up outside the capture
        queue()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                               # one stream: a serial chain of launches
        queue()
    for scene in (other, mesh):
        for dst, src in zip(t, upload(scene, dev)):
            dst.copy_(src)                                                      # in place: the captured pointers
        eager = simplify.simplify_mesh(*(x.clone() for x in t), voxel_size=voxel, return_index=True)
        ws.fill_(0x5a)
        graph.replay()
        torch.cuda.synchronize()
        hdr = ws[:16].view(torch.int32).tolist()
        assert hdr == [eager[0].shape[0], eager[2].shape[0], 0, 0], hdr
        out = [torch.empty_like(e) for e in eager]
        assert raw_calls(t, voxel, ws, out)[1](_ffi.stream_ptr()) == 0
        assert same_bytes(host(out), host(eager))
        assert same_bytes(host(eager), list(ST.simplify(*scene, voxel)[:5]))
    assert L.m3_mesh_simplify_launches() == 8
