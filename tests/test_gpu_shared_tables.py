"""GPU: the key table the mesh and cloud passes share (csrc/table_dev.h) where a probe chain runs past the last slot and
goes on at slot 0, and a lookup has to walk that chain - through the four passes that fill such a table, each against
what its own test compares with, as bytes.  The inputs (tests/table_scenes.py) put at least four distinct keys on the last
slot of a 1024-slot table; that is asserted on the host, with a numpy mix64, before any device call.  Every case runs on a
workspace filled with 0xa5 and on one filled with 0x00: the fill kernels and their segment bounds."""
import numpy as np
import pytest
import torch

import cloud_twin as CT
import knn_twin as KT
import simplify_twin as SV
import smooth_twin as ST
import table_scenes as TS
from mast3r_slam import _ffi, cloud, simplify, smooth
from test_gpu_map_export import thin_numpy

pytestmark = pytest.mark.gpu
FILLS = (0xa5, 0x00)


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def raw(t):
    return t.cpu().numpy().tobytes()


def dirty(nbytes, fill, dev):
    return torch.empty(nbytes, dtype=torch.uint8, device=dev).fill_(fill)


def assert_wraps(keys):
    """At least four distinct keys of the table home at its last slot: three of them land at slot 0 and beyond."""
    assert len(TS.last_slot_keys(keys)) >= 4


def test_smooth_topology_with_a_chain_over_the_last_slot(dev):
    mesh = TS.smooth_mesh()
    V, F = mesh[0].shape[0], mesh[2].shape[0]
    assert V == 600 and F <= 170 and int(smooth._ffi.lib().m3_mesh_smooth_ws_bytes(V, F)) > 0
    first = TS.edge_keys(mesh[2][:, 0], mesh[2][:, 1])
    assert_wraps(first)
    assert (TS.home(first) == TS.S - 1).sum() >= 4
    want = ST.topology(mesh[2], V)
    assert (np.flatnonzero(want["degree"]) // 256).max() == 2                   # row starts in all three tiles
    want_v = ST.smooth(mesh[0], mesh[2], iterations=2, method="taubin", fix_boundary=True).tobytes()
    v, c, f = (up(a, dev) for a in mesh)
    outs = []
    for fill in FILLS:
        got = smooth.mesh_topology(f, V, return_edges=True, workspace=dirty(smooth.workspace_bytes(V, F), fill, dev))
        assert [getattr(got, n) for n in ("edges", "boundary_edges", "nonmanifold_edges", "invalid_faces")] == \
               [want[n] for n in ("edges", "boundary_edges", "nonmanifold_edges", "invalid_faces")]
        out = [raw(got.degree), raw(got.boundary), raw(got.edge_rows), raw(got.edge_faces)]
        assert out == [want[n].tobytes() for n in ("degree", "boundary", "edge_rows", "edge_faces")]
        moved = smooth.smooth_mesh(v, c, f, iterations=2, method="taubin", fix_boundary=True,
                                   workspace=dirty(smooth.workspace_bytes(V, F), fill, dev))[0]
        assert raw(moved) == want_v
        outs.append(out + [raw(moved)])
    assert outs[0] == outs[1]


def test_cloud_cells_with_a_chain_over_the_last_slot(dev):
    p, q, r = TS.cloud_points(), TS.cloud_queries(), TS.CLOUD_RADIUS
    M = len(p)
    assert M <= 512 and len(TS.hot_cells()) >= 4
    assert_wraps(TS.cell_keys(CT.cells(p, r)))
    want = CT.neighbors(p, r)
    assert want["out_of_range"] == 0 and want["count"].max() > 2
    k = 8
    want_self, want_cross = KT.knn(KT.ranked(p, r), k), KT.knn(KT.ranked(p, r, q), k)
    assert want_self["found"].max() == k and want_cross["found"].min() < k
    d, dq = up(p, dev), up(q, dev)
    outs = []
    for fill in FILLS:
        ws = lambda: dirty(cloud.workspace_bytes(M), fill, dev)
        got = cloud.cloud_neighbors(d, r, workspace=ws())
        out = [raw(got.count), raw(got.moments)]
        assert out == [want["count"].tobytes(), want["moments"].tobytes()]
        for res, w in ((cloud.cloud_knn(d, k, r, workspace=ws()), want_self), (cloud.cloud_knn(d, k, r, queries=dq, workspace=ws()), want_cross)):
            one = [raw(res.index), raw(res.dist2), raw(res.found)]
            assert one == [w["index"].tobytes(), w["dist2"].tobytes(), w["found"].tobytes()]
            out += one
        outs.append(out)
    assert outs[0] == outs[1]


def test_simplify_cells_with_a_chain_over_the_last_slot(dev):
    mesh = TS.simplify_mesh()
    V, F = mesh[0].shape[0], mesh[2].shape[0]
    assert V <= 512
    cell, _, ok = SV.cells_of(mesh[0], 1.0)
    assert ok.all()
    assert_wraps(TS.cell_keys(cell))
    want = SV.simplify(*mesh, 1.0)
    assert want[5]["sizes"].max() > 1 and want[2].shape[0] > 0
    t = tuple(up(a, dev) for a in mesh)
    outs = []
    for fill in FILLS:
        got = simplify.simplify_mesh(*t, voxel_size=1.0, return_index=True, workspace=dirty(simplify.workspace_bytes(V, F), fill, dev))
        out = [raw(g) for g in got]
        assert [tuple(g.shape) for g in got] == [w.shape for w in want[:5]] and out == [w.tobytes() for w in want[:5]]
        outs.append(out)
    assert outs[0] == outs[1]


def test_map_voxels_with_a_chain_over_the_last_slot(dev):
    p, c, conf = TS.voxel_cloud()
    M = len(p)
    assert M <= 512
    assert_wraps(TS.cell_keys(np.floor(p / np.float32(1.0))))
    rows = thin_numpy(p, conf, np.arange(M), 1.0)
    assert 4 < rows.size < M
    L = _ffi.lib()
    ws_bytes = int(L.m3_map_voxel_ws_bytes(M))
    assert int(L.m3_map_voxel_table_slots(M)) == TS.S
    dp, dc, dconf = up(p, dev), up(c, dev), up(conf, dev)
    st = _ffi.stream_ptr()
    outs = []
    for fill in FILLS:
        ws = dirty(ws_bytes, fill, dev)
        _ffi.call("m3_map_voxel_count", _ffi.ptr(dp), _ffi.ptr(dconf), M, 1.0, _ffi.ptr(ws), ws_bytes, st)
        m2, dropped = ws[:8].view(torch.int32).tolist()
        assert (m2, dropped) == (rows.size, 0)
        p2 = torch.empty((m2, 3), dtype=torch.float32, device=dev)
        c2 = torch.empty((m2, 3), dtype=torch.uint8, device=dev)
        i2 = torch.empty((m2,), dtype=torch.int64, device=dev)
        _ffi.call("m3_map_voxel_scatter", _ffi.ptr(dp), _ffi.ptr(dc), None, M, _ffi.ptr(ws), ws_bytes, m2, _ffi.ptr(p2), _ffi.ptr(c2),
                  _ffi.ptr(i2), st)
        out = [raw(p2), raw(c2), raw(i2)]
        assert out == [p[rows].tobytes(), c[rows].tobytes(), rows.astype(np.int64).tobytes()]
        outs.append(out)
    assert outs[0] == outs[1]
