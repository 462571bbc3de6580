"""GPU: cloud_neighbors, cloud_normals and remove_radius_outliers (csrc/cloud.hip) against the numpy twin of the header's
rule (tests/cloud_twin.py).  Counts, moments and the filter's selection are compared as bytes: no tolerance.  Normals
are judged against the covariance formed exactly from the twin's integer moments, by the Rayleigh quotient - for every
point that must carry one; nothing is sampled or left out.  The scenes cover cell borders near powers of two with pairs
exactly on the boundary (lattice), negative and offset coordinates (sphere), a cell list longer than a workgroup (ball),
duplicates, isolated points and rows that are not finite (floaters), a rank-one neighbourhood (line) and sizes around
the workgroup (ragged)."""
import numpy as np
import pytest
import torch

import cloud_twin as CT
from mast3r_slam import cloud

pytestmark = pytest.mark.gpu
SCENES = sorted(CT.SCENES)


@pytest.fixture(scope="module")
def twins():
    """scene -> (points, radius, twin outputs), each built once."""
    cache = {}

    def get(name, make=None):
        if name not in cache:
            p, r = (make or CT.SCENES[name])()
            cache[name] = (p, r, CT.neighbors(p, r))
        return cache[name]
    return get


def raw(t):
    return t.cpu().numpy().tobytes()


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def check_neighbors(got, want, moments=True):
    assert got.out_of_range == 0
    assert got.count.dtype == torch.int32 and tuple(got.count.shape) == want["count"].shape and raw(got.count) == want["count"].tobytes()
    if moments:
        assert got.moments.dtype == torch.int64 and tuple(got.moments.shape) == want["moments"].shape
        assert raw(got.moments) == want["moments"].tobytes()
    else:
        assert got.moments is None


@pytest.mark.parametrize("scene", SCENES)
def test_counts_and_moments_equal_the_twin(dev, twins, scene):
    p, r, want = twins(scene)
    M = len(p)
    d = up(p, dev)
    before = d.clone()
    for _ in range(2):                                                          # every call twice
        check_neighbors(cloud.cloud_neighbors(d, r), want)
    check_neighbors(cloud.cloud_neighbors(d, r, moments=False), want, moments=False)
    ws = torch.empty(cloud.workspace_bytes(M) + 64, dtype=torch.uint8, device=dev).fill_(0xa5)
    check_neighbors(cloud.cloud_neighbors(d, r, workspace=ws), want)            # contents ignored on entry
    perm = np.random.default_rng(M).permutation(M)                              # any order of the rows
    got = cloud.cloud_neighbors(up(p[perm], dev), r)
    back = np.empty(M, np.int64)
    back[perm] = np.arange(M)
    check_neighbors(cloud.CloudNeighbors(got.count[up(back, dev)], got.moments[up(back, dev)], got.out_of_range), want)
    assert raw(d) == raw(before)


def check_normals(p, want, normals, variation, toward=None):
    """Every row against the exact covariance of the twin's moments; returns the rows that carry a normal."""
    n32 = normals.cpu().numpy()
    var = variation.cpu().numpy()
    assert n32.dtype == np.float32 and n32.shape == p.shape and var.dtype == np.float32 and var.shape == (len(p),)
    judged = CT.judged(want["count"], want["moments"])
    assert n32[~judged].tobytes() == bytes(12 * int((~judged).sum())) and var[~judged].tobytes() == bytes(4 * int((~judged).sum()))
    if not judged.any():
        return judged
    C = CT.covariance(want["count"], want["moments"])[judged]
    lam = np.linalg.eigvalsh(C)                                                 # ascending
    n = n32[judged].astype(np.float64)
    length = np.linalg.norm(n, axis=1)
    assert np.abs(length - 1.0).max() <= 1e-6
    u = n / length[:, None]
    excess = np.einsum("ia,iab,ib->i", u, C, u) - lam[:, 0]
    bound = 1e-6 * lam[:, 0] + 1e-10 * lam[:, 2]
    worst = int(np.argmax(excess - bound))
    print(f"rows judged {int(judged.sum())}, worst Rayleigh excess {excess[worst]:.3e} against {bound[worst]:.3e}, "
          f"largest excess / bound {np.max(excess / np.maximum(bound, 1e-300)):.3e}")
    assert (excess <= bound).all()
    assert np.abs(var[judged].astype(np.float64) - lam[:, 0] / lam.sum(axis=1)).max() <= 1e-6
    if toward is None:
        top = np.abs(n).max(axis=1, keepdims=True)
        assert ((np.abs(n) == top) & (n > 0)).any(axis=1).all()
    else:
        to = (np.broadcast_to(toward, p.shape)[judged].astype(np.float64) - p[judged].astype(np.float64))
        assert (np.einsum("ia,ia->i", u, to) >= -1e-6 * np.linalg.norm(to, axis=1)).all()
    return judged


@pytest.mark.parametrize("scene", SCENES)
def test_normals_against_the_exact_covariance(dev, twins, scene):
    p, r, want = twins(scene)
    M = len(p)
    d = up(p, dev)
    before = d.clone()
    n, v = cloud.cloud_normals(d, r, return_variation=True)
    judged = check_normals(p, want, n, v)
    if scene in ("plane", "sphere", "ball", "floaters", "line", "ragged1025", "lattice"):
        assert judged.any()
    plain = cloud.cloud_normals(d, r)
    assert isinstance(plain, torch.Tensor) and raw(plain) == raw(n)             # twice, with and without the variation
    one = np.array([0.3, -4.0, 9.0], np.float32)
    n1, v1 = cloud.cloud_normals(d, r, toward=up(one, dev), return_variation=True)
    check_normals(p, want, n1, v1, toward=one)
    assert raw(v1) == raw(v) and raw(n1.abs()) == raw(n.abs())                  # the orientation changes signs only
    each = np.random.default_rng(M + 7).normal(size=(M, 3)).astype(np.float32) * 3
    n2, v2 = cloud.cloud_normals((d, None), r, toward=up(each, dev), return_variation=True)      # the tuple, whole
    check_normals(p, want, n2, v2, toward=each)
    assert raw(n2.abs()) == raw(n.abs()) and raw(cloud.cloud_normals(d, r, toward=up(each, dev))) == raw(n2)
    # min_points: rows below it are zero, the others keep their bytes
    n5 = cloud.cloud_normals(d, r, min_points=5)
    few = up(want["count"] < 5, dev)
    assert not bool(n5[few].any()) and raw(n5[~few]) == raw(n[~few])
    assert raw(d) == raw(before)


def test_flat_plane_normals_are_the_axis(dev, twins):
    p, r, want = twins("flat_plane", CT.flat_plane)
    n = cloud.cloud_normals(up(p, dev), r).cpu().numpy()
    has = want["count"] >= 3
    assert has.sum() > 2900 and np.abs(np.abs(n[has]) - [0, 0, 1]).max() <= 1e-5 and (n[has][:, 2] > 0).all()
    assert not n[~has].any()


def test_sphere_normals_point_inwards(dev, twins):
    p, r, want = twins("sphere")
    centre = CT.SPHERE_CENTRE.astype(np.float32)
    n = cloud.cloud_normals(up(p, dev), r, toward=up(centre, dev)).cpu().numpy().astype(np.float64)
    has = CT.judged(want["count"], want["moments"])
    inward = centre.astype(np.float64) - p[has].astype(np.float64)
    inward /= np.linalg.norm(inward, axis=1, keepdims=True)
    cos = np.einsum("ia,ia->i", n[has], inward)
    print(f"sphere: {int(has.sum())} normals, largest angle to the radius {np.degrees(np.arccos(cos.min())):.2f} degrees")
    assert has.sum() > 2900 and cos.min() >= np.cos(np.radians(15.0))


def test_radius_filter_on_floaters(dev, twins):
    p, r, want = twins("floaters")
    M = len(p)
    g = np.random.default_rng(11)
    c = g.integers(0, 256, size=(M, 3), dtype=np.uint8)
    idx = (7 * np.arange(M) + 3).astype(np.int64)
    dp, dc, di = up(p, dev), up(c, dev), up(idx, dev)
    before = [t.clone() for t in (dp, dc, di)]
    rows = CT.floaters_rows()
    for k in (2, 0, 1, 5, 4000):
        keep = CT.kept_rows(p, r, k, want["count"])
        for _ in range(2):
            out = cloud.remove_radius_outliers(dp, dc, di, radius=r, min_neighbors=k, return_rows=True)
            assert len(out) == 4 and [t.dtype for t in out] == [torch.float32, torch.uint8, torch.int64, torch.int64]
            assert [tuple(t.shape) for t in out] == [(len(keep), 3), (len(keep), 3), (len(keep),), (len(keep),)]
            assert raw(out[0]) == p[keep].tobytes() and raw(out[1]) == c[keep].tobytes()
            assert raw(out[2]) == idx[keep].tobytes() and raw(out[3]) == keep.tobytes()
        whole = cloud.remove_radius_outliers((dp, dc, di), radius=r, min_neighbors=k)          # arity follows the input
        assert len(whole) == 3 and all(raw(a) == raw(b) for a, b in zip(whole, out[:3]))
        pair = cloud.remove_radius_outliers((dp, dc), radius=r, min_neighbors=k)
        assert len(pair) == 2 and raw(pair[0]) == raw(out[0]) and raw(pair[1]) == raw(out[1])
        pair = cloud.remove_radius_outliers(dp, dc, radius=r, min_neighbors=k, return_rows=True)
        assert len(pair) == 3 and raw(pair[2]) == keep.tobytes()
        gone = np.ones(M, bool)
        gone[keep] = False
        if k == 2:                                                              # the floaters and the bad rows, nothing else
            assert np.array_equal(gone, rows["isolated"] | rows["bad"]) and not gone[rows["duplicate"]].any()
        if k == 0:
            assert np.array_equal(gone, rows["bad"])
        if k == 4000:
            assert len(keep) == 0
    assert all(raw(a) == raw(b) for a, b in zip((dp, dc, di), before))


def test_empty_cloud(dev):
    e = torch.empty((0, 3), dtype=torch.float32, device=dev)
    c = torch.empty((0, 3), dtype=torch.uint8, device=dev)
    got = cloud.cloud_neighbors(e, 0.1)
    assert tuple(got.count.shape) == (0,) and tuple(got.moments.shape) == (0, 9) and got.out_of_range == 0
    assert cloud.cloud_neighbors(e, 0.1, moments=False).moments is None
    n, v = cloud.cloud_normals(e, 0.1, return_variation=True)
    assert tuple(n.shape) == (0, 3) and tuple(v.shape) == (0,) and n.dtype == v.dtype == torch.float32
    out = cloud.remove_radius_outliers(e, c, torch.empty((0,), dtype=torch.int64, device=dev), radius=0.1, min_neighbors=1,
                                       return_rows=True)
    assert [tuple(t.shape) for t in out] == [(0, 3), (0, 3), (0,), (0,)]


def test_radius_too_small_for_the_extent(dev):
    p = np.zeros((300, 3), np.float32)
    p[:, 0] = np.linspace(0, 1, 300)
    p[17, 1] = 1.1e-3 * 2 ** 20                                                 # beyond 2^20 cells of edge 1e-3 (1 + 2^-10)
    d = up(p, dev)
    assert CT.neighbors(p, 1e-3)["out_of_range"] == 1
    for call in (lambda: cloud.cloud_neighbors(d, 1e-3), lambda: cloud.cloud_normals(d, 1e-3),
                 lambda: cloud.remove_radius_outliers(d, torch.zeros((300, 3), dtype=torch.uint8, device=dev), radius=1e-3,
                                                      min_neighbors=1)):
        with pytest.raises(ValueError, match="radius too small for the extent of the cloud"):
            call()
    check_neighbors(cloud.cloud_neighbors(d, 2e-3), CT.neighbors(p, 2e-3))      # a little larger: in range again


def test_cpu_tensors_and_other_devices_raise(dev, twins):
    p, r, _ = twins("ragged257")
    with pytest.raises(RuntimeError, match="ROCm device"):
        cloud.cloud_neighbors(torch.from_numpy(p), r)
    d = up(p, dev)
    with pytest.raises(RuntimeError, match="ROCm device"):
        cloud.cloud_normals(d, r, toward=torch.zeros(3))                        # a viewpoint on the host
    with pytest.raises(RuntimeError, match="ROCm device"):
        cloud.remove_radius_outliers(d, torch.zeros((len(p), 3), dtype=torch.uint8), radius=r, min_neighbors=1)
    with pytest.raises(ValueError):
        cloud.cloud_neighbors(d, r, workspace=torch.empty(64, dtype=torch.uint8, device=dev))


def test_graph_replay_gives_the_eager_bytes(dev, twins):
    p, r, want = twins("plane")
    other, _, want2 = twins("plane_seed9", lambda: CT.plane(seed=9))             # as many points, elsewhere
    M = len(p)
    d = up(p, dev)
    toward = up(np.array([0.5, 0.5, 4.0], np.float32), dev)
    ws = torch.empty(cloud.workspace_bytes(M), dtype=torch.uint8, device=dev)
    eager_n, eager_v = (t.clone() for t in cloud.cloud_normals(d, r, toward=toward, return_variation=True, workspace=ws))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                               # warm-up outside the capture
        cloud.cloud_normals(d, r, toward=toward, return_variation=True, workspace=ws)
        cloud.cloud_neighbors(d, r, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                               # one stream: a serial chain of launches
        n, v = cloud.cloud_normals(d, r, toward=toward, return_variation=True, workspace=ws)
        nb = cloud.cloud_neighbors(d, r, workspace=ws)
    assert nb.out_of_range is None                                              # nothing is read back under capture
    for t in (ws, n, v, nb.count, nb.moments):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert raw(n) == raw(eager_n) and raw(v) == raw(eager_v)
    assert raw(nb.count) == want["count"].tobytes() and raw(nb.moments) == want["moments"].tobytes()
    d.copy_(torch.from_numpy(other))                                            # the point contents are overwritten
    ws.fill_(0x5a)
    graph.replay()
    torch.cuda.synchronize()
    assert raw(nb.count) == want2["count"].tobytes() and raw(nb.moments) == want2["moments"].tobytes()
    assert ws[:4].view(torch.int32).item() == 0                                 # the header: no point out of range
    again = cloud.cloud_normals(d, r, toward=toward, return_variation=True)
    assert raw(n) == raw(again[0]) and raw(v) == raw(again[1])
