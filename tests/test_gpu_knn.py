"""GPU: cloud_knn, remove_statistical_outliers and cloud_normals_knn (csrc/cloud.hip) against the numpy twin of the
header's rule (tests/knn_twin.py: brute force over all pairs, no cells).  Every comparison is byte for byte: index, dist2,
found, the filter's q, its sums, its threshold and the rows it keeps, the moments over the k nearest.  The scenes are
those of tests/cloud_twin.py - pairs exactly on the radius and next to powers of two (lattice), negative and offset
coordinates (sphere), a cell list longer than a workgroup (ball), duplicates, isolated points and rows that are not
finite (floaters), a line, sizes around the workgroup (ragged) - and the small ones of the twin: M = 1, 2, k > M - 1, a
pair that differs only in the dropped key bits, 300 exact duplicates.  k = 1, 8, 33, 64 covers the three workgroup sizes
of the query kernel (k <= 16, <= 32, above) and both ends of the range."""
import numpy as np
import pytest
import torch

import cloud_twin as CT
import knn_twin as KT
from mast3r_slam import cloud

pytestmark = pytest.mark.gpu
ALL = {**CT.SCENES, **KT.SMALL}
KS = (1, 8, 33, 64)


@pytest.fixture(scope="module")
def ranked():
    """scene -> (points, radius, the twin's ranking), each built once and never changed."""
    cache = {}

    def get(name):
        if name not in cache:
            p, r = ALL[name]()
            cache[name] = (p, r, KT.ranked(p, r))
        return cache[name]
    return get


def raw(t):
    return t.cpu().numpy().tobytes()


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def check_knn(got, want, k, q):
    assert got.out_of_range == 0
    assert got.index.dtype == torch.int32 and got.dist2.dtype == torch.float32 and got.found.dtype == torch.int32
    assert tuple(got.index.shape) == (q, k) == tuple(got.dist2.shape) and tuple(got.found.shape) == (q,)
    assert raw(got.found) == want["found"].tobytes()
    assert raw(got.index) == want["index"].tobytes()
    assert raw(got.dist2) == want["dist2"].tobytes()


@pytest.mark.parametrize("scene", sorted(ALL))
def test_index_dist2_and_found_equal_the_twin(dev, ranked, scene):
    p, r, rk = ranked(scene)
    M = len(p)
    d = up(p, dev)
    before = d.clone()
    count = cloud.cloud_neighbors(d, r, moments=False).count                    # code that exists: found = min(k, count - 1)
    ws = torch.empty(cloud.workspace_bytes(M) + 64, dtype=torch.uint8, device=dev)
    for k in KS:
        want = KT.knn(rk, k)
        for _ in range(2):                                                      # every call twice
            got = cloud.cloud_knn(d, k, r)
            check_knn(got, want, k, M)
        ws.fill_(0xa5)
        check_knn(cloud.cloud_knn(d, k, r, workspace=ws), want, k, M)           # contents ignored on entry
        assert torch.equal(got.found, torch.clamp(count - 1, min=0, max=k))
    assert raw(d) == raw(before)


@pytest.mark.parametrize("scene", ["plane", "sphere", "ball", "ragged1025"])
def test_row_order_does_not_matter(dev, ranked, scene):
    p, r, rk = ranked(scene)
    M = len(p)
    perm = np.random.default_rng(M + 1).permutation(M)
    back = np.empty(M, np.int64)
    back[perm] = np.arange(M)                                                   # back[old row] = new row
    d = up(p[perm], dev)
    for k in KS:
        # On the CPU first: a row where two of the first k + 1 keys tie in their distance bits is ordered by row there,
        # and a permutation may reorder it - by the rule.  The ball (1999 candidates per query) has one such row at
        # k = 64, the other scenes none; such rows are left out of the comparison, all others are compared.
        tie = KT.distance_bits_tie(rk, k)
        assert tie.sum() <= (1 if scene == "ball" and k == 64 else 0)
        want = KT.knn(rk, k)
        got = cloud.cloud_knn(d, k, r)
        assert raw(got.found[up(back, dev)]) == want["found"].tobytes()
        assert got.dist2[up(back, dev)].cpu().numpy()[~tie].tobytes() == want["dist2"][~tie].tobytes()
        idx = got.index[up(back, dev)].cpu().numpy().astype(np.int64)           # rows of the permuted cloud, in the old query order
        mapped = np.where(idx >= 0, perm[np.maximum(idx, 0)], -1).astype(np.int32)
        assert mapped[~tie].tobytes() == want["index"][~tie].tobytes()


def cross_queries(p, r):
    g = np.random.default_rng(5)
    jitter = (p[::3] + np.float32(0.3 * r) * g.normal(size=p[::3].shape)).astype(np.float32)
    far = (p[:7] + np.float32(40.0 * r)).astype(np.float32)                     # in range, near nothing
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], np.float32)
    return np.concatenate([p[:50], jitter, far, bad])[g.permutation(50 + len(jitter) + 10)]


@pytest.mark.parametrize("scene", ["sphere", "floaters", "lattice", "ragged257"])
def test_cross_mode(dev, ranked, scene):
    p, r, _ = ranked(scene)
    q = cross_queries(p, r)
    d, dq = up(p, dev), up(q, dev)
    before = (d.clone(), dq.clone())
    rk = KT.ranked(p, r, q)
    assert rk["out_of_range"] == 0
    finite = np.isfinite(p).all(axis=1)
    for k in KS:
        want = KT.knn(rk, k)
        for _ in range(2):
            got = cloud.cloud_knn(d, k, r, queries=dq)
            check_knn(got, want, k, len(q))
    copies = np.flatnonzero((q[:, None, :] == p[None, finite][:, :, :]).all(axis=2).any(axis=1))
    assert len(copies) >= 40 and not got.dist2[up(copies, dev), 0].any()        # nothing is excluded: a copy finds its point
    # one query out of range: the call raises, as it does for a point
    q2 = q.copy()
    q2[11] = [0.0, np.float32(1.01 * r * 2 ** 20), 0.0]
    assert KT.ranked(p, r, q2)["out_of_range"] == 1
    with pytest.raises(ValueError, match="radius too small for the extent of the queries"):
        cloud.cloud_knn(d, 8, r, queries=up(q2, dev))
    assert raw(d) == raw(before[0]) and raw(dq) == raw(before[1])


def test_points_out_of_range_and_empty_inputs(dev):
    p = np.zeros((300, 3), np.float32)
    p[:, 0] = np.linspace(0, 1, 300)
    p[17, 1] = 1.1e-3 * 2 ** 20
    d = up(p, dev)
    c = torch.zeros((300, 3), dtype=torch.uint8, device=dev)
    for call in (lambda: cloud.cloud_knn(d, 4, 1e-3), lambda: cloud.cloud_normals_knn(d, 1e-3, 4),
                 lambda: cloud.remove_statistical_outliers(d, c, k=4, radius=1e-3)):
        with pytest.raises(ValueError, match="radius too small for the extent of the cloud"):
            call()
    check_knn(cloud.cloud_knn(d, 4, 2e-3), KT.knn(KT.ranked(p, 2e-3), 4), 4, 300)
    e = torch.empty((0, 3), dtype=torch.float32, device=dev)
    got = cloud.cloud_knn(e, 5, 0.1)
    assert tuple(got.index.shape) == (0, 5) and tuple(got.dist2.shape) == (0, 5) and tuple(got.found.shape) == (0,)
    got = cloud.cloud_knn(e, 5, 0.1, queries=d)                                 # an empty cloud has no neighbours to offer
    assert not got.found.any() and bool((got.index == -1).all()) and bool(torch.isinf(got.dist2).all())
    out = cloud.remove_statistical_outliers(e, c[:0], radius=0.1, return_rows=True, return_stats=True)
    assert [tuple(t.shape) for t in out[:3]] == [(0, 3), (0, 3), (0,)] and out[3]["n"] == 0
    assert tuple(cloud.cloud_normals_knn(e, 0.1, 5).shape) == (0, 3)
    with pytest.raises(RuntimeError, match="ROCm device"):
        cloud.cloud_knn(d.cpu(), 4, 0.1)
    with pytest.raises(ValueError):
        cloud.cloud_knn(d, 4, 0.1, workspace=torch.empty(64, dtype=torch.uint8, device=dev))


@pytest.mark.parametrize("scene", ["sphere", "floaters", "lattice", "line"])
def test_normals_over_64_nearest_are_the_radius_normals(dev, ranked, scene):
    """No point of these scenes has more than 64 others within the radius, so the k = 64 nearest are the whole
    neighbourhood: the new moments kernel must give cloud_neighbors' bytes, and m3_cloud_normals the same normals."""
    p, r, rk = ranked(scene)
    assert rk["ncand"].max() <= 64
    d = up(p, dev)
    want = cloud.cloud_neighbors(d, r)
    toward = up(np.array([0.3, -4.0, 9.0], np.float32), dev)
    n, v, count, mom = cloud.cloud_normals_knn(d, r, 64, toward=toward, return_variation=True, return_moments=True)
    assert count.dtype == torch.int32 and mom.dtype == torch.int64
    assert raw(count) == raw(want.count) and raw(mom) == raw(want.moments)
    n0, v0 = cloud.cloud_normals(d, r, toward=toward, return_variation=True)
    assert raw(n) == raw(n0) and raw(v) == raw(v0)
    assert raw(cloud.cloud_normals_knn((d, None), r, 64, toward=toward)) == raw(n)                    # the tuple, whole; twice
    # k = 8: count = found + 1 and the moments of the twin
    c8, m8 = KT.moments(p, r, KT.knn(rk, 8))
    got = cloud.cloud_normals_knn(d, r, 8, return_moments=True)
    assert raw(got[1]) == c8.tobytes() and raw(got[2]) == m8.tobytes()
    zero = ~got[0].any(dim=1)
    length = got[0].double().norm(dim=1)
    assert bool(((length - 1.0).abs() <= 1e-6)[~zero].all()) and bool(zero[up(c8 < 3, dev)].all())


def three_in_a_row():
    """Only the middle point has two others within the radius: n = 1 at k = 2."""
    return np.array([[0, 0, 0], [0.4, 0, 0], [-0.4, 0, 0]], np.float32), 0.5


STAT_CASES = [(s, k, ratio) for s in ("floaters", "sphere") for k in (4, 20) for ratio in (0.5, 2.0)] + \
             [("three", 2, 2.0), ("five", 8, 2.0), ("pair", 1, 0.5), ("duplicates", 20, 2.0)]


@pytest.mark.parametrize("scene,k,ratio", STAT_CASES)
def test_statistical_filter_equals_the_twin(dev, ranked, scene, k, ratio):
    if scene == "three":
        p, r = three_in_a_row()
        rk = KT.ranked(p, r)
    else:
        p, r, rk = ranked(scene)
    M = len(p)
    g = np.random.default_rng(13)
    c = g.integers(0, 256, size=(M, 3), dtype=np.uint8)
    idx = (5 * np.arange(M) + 2).astype(np.int64)
    q = KT.isqrt_sum(p, r, KT.knn(rk, k), k)
    want = KT.statistics(q, ratio)
    keep = want["kept"]
    dp, dc, di = up(p, dev), up(c, dev), up(idx, dev)
    before = [t.clone() for t in (dp, dc, di)]
    for _ in range(2):
        out = cloud.remove_statistical_outliers(dp, dc, di, k=k, std_ratio=ratio, radius=r, return_rows=True, return_stats=True)
        assert len(out) == 5 and [t.dtype for t in out[:4]] == [torch.float32, torch.uint8, torch.int64, torch.int64]
        st = out[4]
        assert st["q"].dtype == torch.int32 and raw(st["q"]) == q.tobytes()
        assert (st["n"], st["S1"], st["S2"]) == (want["n"], want["S1"], want["S2"]) and st["T"] == want["T"]
        assert raw(out[3]) == keep.tobytes()
        assert raw(out[0]) == p[keep].tobytes() and raw(out[1]) == c[keep].tobytes() and raw(out[2]) == idx[keep].tobytes()
    whole = cloud.remove_statistical_outliers((dp, dc, di), k=k, std_ratio=ratio, radius=r)            # arity follows the input
    assert len(whole) == 3 and all(raw(a) == raw(b) for a, b in zip(whole, out[:3]))
    pair = cloud.remove_statistical_outliers(dp, dc, k=k, std_ratio=ratio, radius=r)
    assert len(pair) == 2 and raw(pair[0]) == raw(out[0]) and raw(pair[1]) == raw(out[1])
    gone = np.ones(M, bool)
    gone[keep] = False
    if scene == "floaters":
        rows = CT.floaters_rows()
        assert gone[rows["isolated"]].all() and gone[rows["bad"]].all()         # no neighbour at all: never complete
        if (k, ratio) == (4, 2.0):
            assert (q[rows["duplicate"]] >= 0).all() and not gone[rows["duplicate"]].any()       # a neighbour at distance 0
        assert 0 < len(keep) < M
    if scene == "sphere":
        assert 0 < len(keep) < M
    if scene == "three":
        assert want["n"] == 1 and keep.tolist() == [0]                          # n < 2: var = 0, T = q
    if scene == "five":
        assert want["n"] == 0 and len(keep) == 0 and st["T"] < 0                # nothing is complete: an empty cloud
    if scene == "duplicates":
        assert (q[(p == np.array([0.3, 0.7, -0.2], np.float32)).all(axis=1)] == 0).all() and len(keep) >= 300
    assert all(raw(a) == raw(b) for a, b in zip((dp, dc, di), before))


def test_graph_replay_gives_the_eager_bytes(dev, ranked):
    p, r, rk = ranked("plane")
    other, _ = CT.plane(seed=9)                                                 # as many points, elsewhere
    M, k = len(p), 8
    d = up(p, dev)
    ws = torch.empty(cloud.workspace_bytes(M), dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                               # warm-up outside the capture
        cloud.cloud_knn(d, k, r, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                               # one stream: a serial chain of seven launches
        got = cloud.cloud_knn(d, k, r, workspace=ws)
    assert got.out_of_range is None                                             # nothing is read back under capture
    for t in (ws, got.index, got.dist2, got.found):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    check_knn(cloud.KnnResult(got.index, got.dist2, got.found, 0), KT.knn(rk, k), k, M)
    d.copy_(torch.from_numpy(other))
    ws.fill_(0x5a)
    graph.replay()
    torch.cuda.synchronize()
    check_knn(cloud.KnnResult(got.index, got.dist2, got.found, 0), KT.knn(KT.ranked(other, r), k), k, M)
    assert ws[:16].view(torch.int32).tolist() == [0, M, 0, 0]
