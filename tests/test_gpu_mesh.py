"""GPU: the mesh kernels (csrc/mesh.hip) through export.collect_mesh, against the numpy restatement of the rule in
tests/mesh_twin.py (its docstring states the rule word for word).  Faces, the vertex selection and its order, colours
and indices are exact; vertices are the exporter's bytes and carry its 1e-5 bound against float64."""
import numpy as np
import pytest
import torch

import mesh_twin as MT
from mast3r_slam import _ffi, export

pytestmark = pytest.mark.gpu


def run(frames, thr, stride, ratio):
    out = export.collect_mesh(frames, c_conf_threshold=thr, stride=stride, edge_ratio=ratio, return_index=True)
    return [t.cpu().numpy() for t in out]


def check(sc, dev, thr, stride, ratio, frames=None, bound=1e-5):
    """Every property of the issue's list for one scene and parameter set; returns the outputs.  bound: on |v - v64|, the
    exporter's 1e-5 for unit-scale data."""
    frames = frames or MT.frames_of(sc, dev)
    v, c, f, i = run(frames, thr, stride, ratio)
    want_f, want_i, cand = MT.mesh_twin(sc, thr, stride, ratio)
    print(f"K={sc['K']} {sc['H']}x{sc['W']} {sc['layout']} thr={thr} stride={stride} ratio={ratio}: "
          f"{want_f.shape[0]} of {cand} faces, {want_i.size} vertices")
    assert v.dtype == np.float32 and c.dtype == np.uint8 and f.dtype == np.int32 and i.dtype == np.int64
    assert v.shape == (want_i.size, 3) and c.shape == (want_i.size, 3) and f.shape == (want_f.shape[0], 3)
    assert np.array_equal(i, want_i)                                            # the used vertices, ascending
    if i.size > 1:
        assert (np.diff(i) > 0).all()
    if f.size:
        assert f.min() >= 0 and f.max() < v.shape[0]
        assert np.array_equal(i[f], want_f)                                     # the twin's triples, in order
        assert np.array_equal(np.unique(f), np.arange(v.shape[0]))              # no vertex is unreferenced
    assert np.array_equal(c, MT.colours(sc)[i])
    p, _, pi = [t.cpu().numpy() for t in export.collect_map(frames, c_conf_threshold=thr, return_index=True)]
    rows = np.searchsorted(pi, i)
    assert i.size == 0 or (rows.max() < pi.size and np.array_equal(pi[rows], i))  # every mesh vertex is an exported point
    assert v.tobytes() == p[rows].tobytes()
    err = np.abs(v - MT.world64(sc)[i]).max() if i.size else 0.0
    print(f"    max |v - v64| = {err:.3g}")
    assert err < bound
    again = run(frames, thr, stride, ratio)
    for a, b in zip((v, c, f, i), again):
        assert a.tobytes() == b.tobytes()
    v3, c3, f3 = export.collect_mesh(frames, c_conf_threshold=thr, stride=stride, edge_ratio=ratio)   # without the index
    assert v3.cpu().numpy().tobytes() == v.tobytes() and c3.cpu().numpy().tobytes() == c.tobytes()
    assert f3.cpu().numpy().tobytes() == f.tobytes()
    return v, c, f, i


@pytest.mark.parametrize("layout", ["f32", "u8"])
@pytest.mark.parametrize("name", ["33x65", "33x65 stride 2", "33x65 stride 3", "33x65 no threshold", "64x128", "10x530",
                                  "10x530 stride 2"])
def test_faces_vertices_colours_order(dev, name, layout):
    """33x65: nothing aligned, N % 4 != 0, scalar loads, a keyframe without faces in the middle; 64x128: 16-byte loads;
    10x530: three row segments per grid row, and 16-byte loads whose rows start at every offset within a group."""
    sc, thr, stride, ratio = MT.case_scene(name, layout)
    v, c, f, i = check(sc, dev, thr, stride, ratio)
    assert f.shape[0] > 0


@pytest.mark.parametrize("layout", ["f32", "u8"])
def test_one_cell(dev, layout):
    v, c, f, i = check(MT.one_cell_scene(layout), dev, MT.THR, 1, 0.8)
    assert f.tolist() == [[0, 2, 1]] and i.tolist() == [0, 1, 2]


@pytest.mark.parametrize("layout", ["f32", "u8"])
def test_more_cell_row_segments_than_one_scan_round(dev, layout):
    """4099 face segments: the scan of the segment counts takes a second round of 4096, and faces lie beyond it."""
    sc = MT.tall_scene(layout)
    want_f, _, cand = MT.mesh_twin(sc, MT.THR, 1, 0.05)
    beyond = int((want_f[:, 0] // sc["W"] >= 4096).sum())                       # a triangle's first vertex is in its cell row
    print(f"{want_f.shape[0]} of {cand} faces, {beyond} in cell rows >= 4096")
    assert beyond >= 1
    # f = W = 5 and 4100 rows: |y / z| reaches 410 and |X| about 900, against about 5 in the data the exporter's 1e-5 was
    # set for (test_gpu_map_export.py: normal coordinates).  The same relative bound here; the vertices are still the
    # exporter's bytes, exactly.
    reach = float(np.abs(sc["X"][np.isfinite(sc["X"])]).max())
    assert reach > 5.0
    check(sc, dev, MT.THR, 1, 0.05, bound=1e-5 * reach / 5.0)


def test_an_edge_on_the_bound_is_kept_and_one_an_ulp_past_it_dropped(dev):
    v, c, f, i = check(MT.bound_scene(), dev, MT.THR, 1, 0.5)
    assert i[f].tolist() == [[0, 2, 1]]                                         # keyframe 0's (a, c, b); keyframe 1 has none


@pytest.mark.parametrize("H,W", [(1, 8), (8, 1)])
def test_no_cells_gives_empty_outputs_of_the_right_types(dev, H, W):
    sc = MT.make_scene(1, H, W, seed=2, layout="f32")
    sc["C"][:] = 2.0 * sc["Nk"][:, None]
    v, c, f, i = check(sc, dev, MT.THR, 1, 10.0)
    assert v.shape == (0, 3) and c.shape == (0, 3) and f.shape == (0, 3) and i.shape == (0,)
    check(sc, dev, MT.THR, 9, 10.0)                                             # a stride beyond the image: one vertex


@pytest.mark.parametrize("thr,ratio", [(float("inf"), 0.05), (MT.THR, 1e-4)])
def test_nothing_survives(dev, thr, ratio):
    """No valid vertex, or no edge short enough: empty outputs, and no scatter is launched."""
    sc, _, stride, _ = MT.case_scene("33x65")
    v, c, f, i = check(sc, dev, thr, stride, ratio)
    assert v.shape == (0, 3) and f.shape == (0, 3) and f.dtype == np.int32


def test_unaligned_views_give_the_same_mesh(dev):
    """X / C / image views that start one element into their allocation: no 16-byte load is possible, the result is the
    aligned scene's.  64x128 takes 16-byte loads when aligned, 33x65 never does."""
    for name in ("33x65", "64x128"):
        sc, thr, stride, ratio = MT.case_scene(name)
        ref = run(MT.frames_of(sc, dev), thr, stride, ratio)
        frames = MT.frames_of(sc, dev, offset=1)
        assert all(f.X_canon.data_ptr() % 16 and f.C.data_ptr() % 16 and f.img.data_ptr() % 16 for f in frames)
        got = check(sc, dev, thr, stride, ratio, frames=frames)
        for a, b in zip(ref, got):
            assert a.tobytes() == b.tobytes()


def test_a_keyframe_alone_gives_its_faces_minus_the_row_offset(dev):
    sc, thr, stride, ratio = MT.case_scene("33x65 middle")
    frames = MT.frames_of(sc, dev)
    v, c, f, i = check(sc, dev, thr, stride, ratio, frames=frames)
    N = sc["H"] * sc["W"]
    mine = (i >= N) & (i < 2 * N)
    first = int(np.argmax(mine))
    fk = f[(f[:, 0] >= first) & (f[:, 0] < first + mine.sum())]
    va, ca, fa, ia = run(frames[1:2], thr, stride, ratio)
    assert fa.shape[0] > 0 and np.array_equal(fa, fk - first)
    assert np.array_equal(ia, i[mine] - N) and va.tobytes() == v[mine].tobytes() and ca.tobytes() == c[mine].tobytes()


def test_the_scatter_call_replays_from_a_graph(dev):
    """With V and F known the scatter call queues launches only: it captures into a graph, and the replay writes the
    eager call's bytes."""
    L = _ffi.lib()
    sc, thr, stride, ratio = MT.case_scene("64x128")
    frames = MT.frames_of(sc, dev)
    want = export.collect_mesh(frames, c_conf_threshold=thr, stride=stride, edge_ratio=ratio, return_index=True)
    m = export._map_tables(frames)                                              # host-to-device copies stay outside the capture
    K, H, W = sc["K"], sc["H"], sc["W"]
    ws_bytes = int(L.m3_mesh_ws_bytes(K, H, W, stride))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    V, F = want[0].shape[0], want[2].shape[0]
    out = [torch.empty_like(t) for t in want]

    def count():
        _ffi.call("m3_mesh_count", _ffi.ptr(m.table[0]), _ffi.ptr(m.table[1]), _ffi.ptr(m.poses), _ffi.ptr(m.nk), K, H, W,
                  stride, 1, thr, ratio, _ffi.ptr(ws), ws_bytes, _ffi.stream_ptr())

    def scatter():
        _ffi.call("m3_mesh_scatter", _ffi.ptr(m.table[0]), _ffi.ptr(m.table[1]), _ffi.ptr(m.table[2]), _ffi.ptr(m.poses),
                  _ffi.ptr(m.nk), K, H, W, stride, 1, thr, ratio, m.layout, _ffi.ptr(ws), ws_bytes, V, F, _ffi.ptr(out[0]),
                  _ffi.ptr(out[1]), _ffi.ptr(out[2]), _ffi.ptr(out[3]), _ffi.stream_ptr())

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                               # warm-up outside the capture
        count()
        scatter()
    torch.cuda.current_stream().wait_stream(side)
    assert ws[:8].view(torch.int32).tolist() == [V, F]
    assert all(torch.equal(a, b) for a, b in zip(out, want))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                               # one stream: a serial chain of launches
        scatter()
    for _ in range(2):
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, want))
