"""GPU: icp_sums and register_clouds (csrc/icp.hip) against the numpy twin of the header's rule (tests/icp_twin.py).
Every comparison is byte for byte: the pair count, the 36 sums, the correspondences, the state block, the history and T.
The scenes are the twin's - a bumpy sheet, a closed box, a flat plane, each with duplicated target points, zero and NaN
normals - and every source of 16 rows or more holds a NaN row, rows far from the target and a row out of cell range.
Source sizes 1, 255, 256, 257, 513 cover the tile of 256 rows from both sides; 65 537 rows are 257 tiles, so that slot 0
of the second stage adds two of them."""
import ctypes

import numpy as np
import pytest
import torch

import icp_twin as IT
from mast3r_slam import _ffi, cloud, register

pytestmark = pytest.mark.gpu
SIZES = (1, 255, 256, 257, 513, 65537)
METHODS = ("point_to_point", "point_to_plane")


@pytest.fixture(scope="module")
def scenes():
    return {k: f() for k, f in IT.SCENES.items()}


def raw(t):
    return t.cpu().numpy().tobytes()


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def source_of(sc, ns):
    if ns <= 1024:
        return IT.make_source(sc, ns)
    base, M = IT.make_source(sc, 700)
    return base[np.arange(ns) % len(base)], M


def near(M, seed):
    """A pose a little off inv(M): what an iteration on the way sees."""
    g = np.random.default_rng(seed)
    return IT.matrix_of(IT.update(IT.pose_of(np.linalg.inv(M)), (0.004 * g.normal(size=7)).tolist()))


@pytest.mark.parametrize("ns", SIZES)
@pytest.mark.parametrize("scene", sorted(IT.SCENES))
def test_sums_equal_the_twin(dev, scenes, scene, ns):
    sc = scenes[scene]
    src, M = source_of(sc, ns)
    T = near(M, ns)
    pose = register._pose(T)
    s, t, n = up(src, dev), up(sc["target"], dev), up(sc["normals"], dev)
    before = [x.clone() for x in (s, t, n)]
    nt = len(sc["target"])
    ws = torch.empty(register.registration_workspace_bytes(ns, nt, 0), dtype=torch.uint8, device=dev)
    host = (ctypes.c_double * 13)(*pose.tolist())
    for mode, method in enumerate(METHODS):
        want = IT.sums(src, sc["target"], sc["radius"], pose, sc["normals"], mode)
        H, g, cost = IT.unpack(want["sums"])
        if ns >= 255:
            assert want["count"][0] > 0.8 * ns * (0.9 if mode else 1)            # the case is not empty
        for _ in range(2):                                                      # the entry point, on a filled workspace, twice
            ws.fill_(0xa5)
            count = torch.full((3,), -1, dtype=torch.int64, device=dev)
            sums = torch.full((36,), np.nan, dtype=torch.float64, device=dev)
            pairs = torch.full((ns,), -7, dtype=torch.int32, device=dev)
            _ffi.call("m3_icp_sums", s.data_ptr(), ns, t.data_ptr(), n.data_ptr(), nt, float(np.float32(sc["radius"])), mode,
                      ctypes.addressof(host), count.data_ptr(), sums.data_ptr(), pairs.data_ptr(), ws.data_ptr(), ws.numel(),
                      _ffi.stream_ptr())
            assert count.tolist() == want["count"].tolist()
            assert raw(sums) == want["sums"].tobytes() and raw(pairs) == want["pairs"].tobytes()
        got = register.icp_sums(s, t, sc["radius"], T, n, method, return_pairs=True)       # and through the module
        assert [got.count, got.finite, got.out_of_range] == want["count"].tolist()
        assert got.H.tobytes() == H.tobytes() and got.g.tobytes() == g.tobytes()
        assert np.float64(got.cost).tobytes() == np.float64(cost).tobytes()
        assert got.pairs.dtype == torch.int32 and raw(got.pairs) == want["pairs"].tobytes()
    # the correspondences are cloud_knn's for the moved rows, where that call accepts them (no row out of range)
    ok = np.flatnonzero(np.isfinite(want["q32"]).all(axis=1) & (np.abs(want["q32"]) < 1e3).all(axis=1))
    knn = cloud.cloud_knn(t, 1, sc["radius"], queries=up(want["q32"][ok], dev))
    assert raw(knn.index[:, 0]) == want["pairs"][ok].tobytes()
    assert all(raw(a) == raw(b) for a, b in zip((s, t, n), before))


def run(dev, src, sc, ws_fill=0xa5, **kw):
    """(Registration, state float64 [24], history bytes of all `iterations` rows) of a call on a filled workspace."""
    it = kw.get("iterations", 30)
    nt = len(sc["target"])
    ws = torch.full((register.registration_workspace_bytes(len(src), nt, it),), ws_fill, dtype=torch.uint8, device=dev)
    normals = up(sc["normals"], dev) if kw.pop("normals", True) else None
    reg = register.register_clouds(up(src, dev), up(sc["target"], dev), sc["radius"], normals, workspace=ws, return_pairs=True, **kw)
    at = register._state_offset(nt)
    blob = ws[at:at + 8 * (24 + 5 * it)].cpu().numpy()
    return reg, blob[:192].view(np.float64), blob[192:].tobytes()


def check(reg, state, hist, want, it, fill=0xa5):
    ran = int(want["state"][IT.S_ITERS])
    assert state.tobytes() == want["state"].tobytes()
    assert hist[:40 * ran] == want["history"].tobytes()
    assert hist[40 * ran:] == bytes([fill]) * (40 * (it - ran))                 # rows of iterations that did not run: untouched
    assert reg.T.tobytes() == want["T"].tobytes() and reg.history.tobytes() == want["history"].tobytes()
    assert raw(reg.pairs) == want["pairs"].tobytes()
    st = want["state"]
    assert (reg.iterations, reg.converged, reg.status) == (ran, bool(st[IT.S_DONE]), register.STATUS[int(st[IT.S_STATUS])])
    assert reg.scale == st[12] and reg.out_of_range == st[IT.S_FAR]
    assert reg.fitness == (st[IT.S_EVAL_PAIRS] / st[IT.S_FINITE] if st[IT.S_FINITE] else 0.0)


@pytest.mark.parametrize("with_scale", (False, True))
@pytest.mark.parametrize("iterations", (0, 1, 8, 30))
@pytest.mark.parametrize("scene,method", (("sheet", "point_to_plane"), ("box", "point_to_point")))
def test_registration_equals_the_twin(dev, scenes, scene, method, iterations, with_scale):
    sc = scenes[scene]
    src, M = IT.make_source(sc, 513)
    mode = METHODS.index(method)
    want = IT.register(src, sc["target"], sc["radius"], sc["normals"], mode, with_scale=with_scale, iterations=iterations)
    reg, state, hist = run(dev, src, sc, method=method, with_scale=with_scale, iterations=iterations)
    check(reg, state, hist, want, iterations)
    if iterations == 30:                                                        # early stop
        assert reg.converged and reg.iterations < 30 and reg.status == "ok"
        if with_scale:
            assert IT.pose_error(reg.T, M) < 1e-7
    again, state2, hist2 = run(dev, src, sc, method=method, with_scale=with_scale, iterations=iterations)
    assert state2.tobytes() == state.tobytes() and hist2 == hist and raw(again.pairs) == raw(reg.pairs)


def test_failures_and_empty_clouds(dev, scenes):
    sc = scenes["plane"]
    src, M = IT.make_source(sc, 300)
    T0 = near(M, 1)
    pose = register._pose(T0)
    # the flat plane in plane mode cannot see in-plane motion: singular, and the pose is the initial one
    want = IT.register(src, sc["target"], sc["radius"], sc["normals"], 1, pose=pose, with_scale=True, iterations=8)
    reg, state, hist = run(dev, src, sc, T_init=T0, with_scale=True, iterations=8)
    check(reg, state, hist, want, 8)
    assert reg.status == "singular" and reg.iterations == 1 and not reg.converged and reg.T.tobytes() == IT.matrix_of(pose).tobytes()
    # fewer matches than min_pairs
    want = IT.register(src[:12], sc["target"], sc["radius"], None, 0, iterations=8)
    reg, state, hist = run(dev, src[:12], sc, normals=False, iterations=8)
    check(reg, state, hist, want, 8)
    assert reg.status == "too_few_pairs" and reg.iterations == 1 and reg.history[0, 0] == 8
    # min_pairs = 8 lets the same rows through
    want = IT.register(src[:12], sc["target"], sc["radius"], None, 0, iterations=3, min_pairs=8)
    reg, state, hist = run(dev, src[:12], sc, normals=False, iterations=3, min_pairs=8)
    check(reg, state, hist, want, 3)
    assert reg.status == "ok" and reg.iterations == 3
    # a start so far off that nothing matches
    far = np.eye(4)
    far[:3, 3] = [50.0, 0.0, 0.0]
    want = IT.register(src, sc["target"], sc["radius"], sc["normals"], 1, pose=register._pose(far), iterations=4)
    reg, state, hist = run(dev, src, sc, T_init=far, iterations=4)
    check(reg, state, hist, want, 4)
    assert reg.status == "too_few_pairs" and reg.fitness == 0.0 and reg.inlier_rmse == 0.0 and (reg.pairs == -1).all()
    # empty source, empty target
    empty = dict(target=np.zeros((0, 3), np.float32), normals=np.zeros((0, 3), np.float32), radius=sc["radius"])
    for s_, sc_ in ((src[:0], sc), (src, empty), (src[:0], empty)):
        for method in METHODS:
            want = IT.register(s_, sc_["target"], sc_["radius"], sc_["normals"], METHODS.index(method), iterations=2)
            reg, state, hist = run(dev, s_, sc_, method=method, iterations=2)
            check(reg, state, hist, want, 2)
            assert reg.status == "too_few_pairs" and tuple(reg.pairs.shape) == (len(s_),)
    got = register.icp_sums(up(src[:0], dev), up(sc["target"], dev), sc["radius"], None)
    assert got.count == 0 and not got.H.any() and got.cost == 0.0


def test_graph_replay_gives_the_eager_bytes(dev, scenes):
    sc, other = scenes["sheet"], scenes["box"]
    nt = min(len(sc["target"]), len(other["target"]))
    src, _ = IT.make_source(sc, 513)
    src2, _ = IT.make_source(other, 513)
    s, t, n = up(src, dev), up(sc["target"][:nt], dev), up(sc["normals"][:nt], dev)
    it = 12
    ws = torch.empty(register.registration_workspace_bytes(513, nt, it), dtype=torch.uint8, device=dev)
    kw = dict(with_scale=True, iterations=it, return_pairs=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                               # warm-up outside the capture
        register.register_clouds(s, t, sc["radius"], n, workspace=ws, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                               # one stream: a serial chain of launches
        got = register.register_clouds(s, t, sc["radius"], n, workspace=ws, **kw)
    assert got.T is None and got.status is None                                 # nothing is read back under capture
    at = register._state_offset(nt)
    span = slice(at, at + 8 * (24 + 5 * it))
    for scene, source in ((sc, src), (other, src2)):                            # the second round: new inputs, same graph
        s.copy_(torch.from_numpy(source))
        t.copy_(torch.from_numpy(scene["target"][:nt]))
        n.copy_(torch.from_numpy(scene["normals"][:nt]))
        ws.fill_(0x5a)
        got.pairs.zero_()
        graph.replay()
        torch.cuda.synchronize()
        replayed = register.read_registration(ws, 513, nt, it, got.pairs)
        ws2 = torch.full_like(ws, 0x5a)
        eager = register.register_clouds(s, t, sc["radius"], n, workspace=ws2, **kw)
        assert raw(ws[span]) == raw(ws2[span]) and raw(replayed.pairs) == raw(eager.pairs)
        assert replayed.T.tobytes() == eager.T.tobytes() and replayed.iterations == eager.iterations and eager.status == "ok"
        want = IT.register(source, scene["target"][:nt], sc["radius"], scene["normals"][:nt], 1, with_scale=True, iterations=it)
        assert eager.T.tobytes() == want["T"].tobytes()
    assert _ffi.lib().m3_icp_launches(it) == 6 + 2 * it + 2
