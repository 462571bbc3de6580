"""CPU: the k-nearest-neighbour rule (tests/knn_twin.py) against things that do not come from the twin - a plain argsort
of the distances where nothing ties, the packed key on cases written out by hand, the integer square root and the
threshold by hand; the host checks of mast3r_slam/cloud.py that need no device; and the exports, the launch count and the
argument validation of the C entry points, which happen before any HIP call."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

import cloud_twin as CT
import knn_twin as KT
from mast3r_slam import _ffi, cloud, mast3r_utils

SCENES = {**CT.SCENES, **KT.SMALL}


@pytest.fixture(scope="module")
def built_lib():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(_ffi.LIB_PATH):
        spec = importlib.util.spec_from_file_location("m3build", os.path.join(root, "mast3r-slam_amd", "build.py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        m.build(verbose=False)
    return ctypes.CDLL(_ffi.LIB_PATH)


# ---- the twin --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_twin_against_a_plain_argsort(scene):
    """Row by row, no keys: the candidates by the radius test, ordered by a stable argsort of d2 itself.  Where no two
    of a row's first k + 1 distances are equal and no two keys tie in their distance bits, the rows are the twin's."""
    p, r = SCENES[scene]()
    r32 = float(np.float32(r))
    rk = KT.ranked(p, r)
    assert rk["out_of_range"] == 0
    P = p.astype(np.float64)
    finite = np.isfinite(p).all(axis=1)
    count = CT.brute_counts(p, r)
    compared = 0
    for k in (1, 8, 33, 64):
        got = KT.knn(rk, k)
        assert got["index"].dtype == np.int32 and got["dist2"].dtype == np.float32 and got["found"].dtype == np.int32
        assert np.array_equal(got["found"], np.minimum(k, np.maximum(count.astype(np.int64) - 1, 0)))
        tie = KT.distance_bits_tie(rk, k)
        for i in range(0, len(p), 7):                                           # every seventh row: the loop is the slow part
            if not finite[i]:
                assert got["found"][i] == 0 and (got["index"][i] == -1).all() and np.isinf(got["dist2"][i]).all()
                continue
            d = P - P[i]
            with np.errstate(invalid="ignore"):
                d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                cand = np.flatnonzero((d2 <= r32 * r32) & finite & (np.arange(len(p)) != i))
            order = cand[np.argsort(d2[cand], kind="stable")][:k + 1]
            n = got["found"][i]
            assert n == min(k, len(cand))
            assert (got["index"][i, n:] == -1).all() and np.isinf(got["dist2"][i, n:]).all()
            if tie[i] or len(np.unique(d2[order])) != len(order):
                assert sorted(got["dist2"][i, :n].tolist()) == got["dist2"][i, :n].tolist()
                continue
            assert got["index"][i, :n].tolist() == order[:n].tolist()
            assert got["dist2"][i, :n].tobytes() == d2[order[:n]].astype(np.float32).tobytes()
            compared += 1
    if scene in ("plane", "sphere", "ball", "floaters", "ragged1025", "ragged257"):
        assert compared > 100                                                   # the random scenes are tie-free


def test_packed_key_by_hand():
    key = lambda d2, j: int(KT.pack_key(np.array([d2]), np.array([j]))[0])
    assert key(0.0, 0) == 0 and key(0.0, 5) == 5
    assert key(1.0, 3) == (0x3ff << 52) | 3 and key(2.0, 2 ** 30 - 1) == (0x400 << 52) | (2 ** 30 - 1)
    # the last kept bit is mantissa bit 30: 1 + 2^-22 differs from 1, 1 + 2^-23 does not
    assert key(1.0 + 2.0 ** -22, 0) == (0x3ff << 52) | (1 << 30) and key(1.0 + 2.0 ** -23, 0) == key(1.0, 0)
    assert key(1.0 + 2.0 ** -23, 1) > key(1.0, 0) and key(1.0, 1) > key(1.0 + 2.0 ** -23, 0)     # ordered by row
    assert key(1.0 + 2.0 ** -22, 0) > key(1.0, 2 ** 30 - 1)                     # a kept bit beats any row
    # monotone over exponents and denormals: the order of non-negative doubles is the order of their bits
    vals = [0.0, 5e-324, 1e-310, 2.2250738585072014e-308, 1e-30, 0.1, 0.5, 1.0, 1.5, 1e30]
    keys = [key(v, 7) for v in vals]
    assert keys == sorted(keys) and keys[1] == keys[0]                          # the smallest denormal: dropped bits only
    assert int(KT.ROW_MASK) == 2 ** 30 - 1


def test_dropped_bits_scene_is_what_it_says():
    p, r = KT.dropped_bits()
    d2 = (p[:2, 0].astype(np.float64)) ** 2
    assert d2[0] > d2[1] and d2[1] == 0.5625
    assert int(KT.pack_key(d2[:1], [0])[0]) >> 30 == int(KT.pack_key(d2[1:], [1])[0]) >> 30
    got = KT.knn(KT.ranked(p, r), 2)
    assert got["index"][2].tolist() == [0, 1]                                   # the farther point first: the lower row
    assert got["dist2"][2, 0] > got["dist2"][2, 1]                              # and dist2 says so
    assert got["index"][0].tolist() == [1, 2] and got["index"][1].tolist() == [0, 2]


def test_small_scenes_by_hand():
    one = KT.knn(KT.ranked(*KT.single()), 3)
    assert one["found"].tolist() == [0] and one["index"].tolist() == [[-1, -1, -1]] and np.isinf(one["dist2"]).all()
    two = KT.knn(KT.ranked(*KT.pair()), 2)
    assert two["found"].tolist() == [1, 1] and two["index"].tolist() == [[1, -1], [0, -1]]
    assert two["dist2"][:, 0].tolist() == [0.0625, 0.0625]
    five = KT.knn(KT.ranked(*KT.five()), 8)                                     # k > M - 1; point 3 exactly on point 0's boundary
    assert five["found"].tolist() == [3, 2, 2, 1, 0]
    assert five["index"][0, :3].tolist() == [2, 1, 3] and five["dist2"][0, :3].tolist() == [0.0625, 0.25, 1.0]
    p, r = KT.duplicates()
    rk = KT.ranked(p, r)
    same = np.flatnonzero((p == np.array([0.3, 0.7, -0.2], np.float32)).all(axis=1))
    assert len(same) == 300
    got = KT.knn(rk, 64)
    for i in same[:5]:                                                          # 299 candidates at distance 0: the lowest rows
        assert got["index"][i].tolist() == [j for j in same if j != i][:64] and not got["dist2"][i].any()
    assert KT.distance_bits_tie(rk, 64)[same].all()


def test_cross_mode_of_the_twin():
    p, r = CT.sphere()
    q = np.concatenate([p[:5], p[:3] + np.float32(0.01), [[np.nan, 0, 0]], [[1e9, 0, 0]], [[50.0, 50.0, 50.0]]]).astype(np.float32)
    rk = KT.ranked(p, r, q)
    assert rk["out_of_range"] == 1
    got = KT.knn(rk, 4)
    assert got["index"][:5, 0].tolist() == [0, 1, 2, 3, 4] and not got["dist2"][:5, 0].any()        # nothing is excluded
    assert got["found"][8:].tolist() == [0, 0, 0]


def test_integer_square_root_sum_and_threshold_by_hand():
    p = np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.25, 0], [0, 0, -1], [2, 0, 0]], np.float32)
    nn = KT.knn(KT.ranked(p, 1.0), 2)
    q = KT.isqrt_sum(p, 1.0, nn, 2)
    # r = 1: D = d2 2^32, s = sqrt(d2) 2^16.  Point 0: 0.25 + 0.5; point 1: 0.5 + sqrt(0.3125); point 2: 0.25 + sqrt(0.3125)
    s = math.isqrt(int(0.3125 * 2 ** 32))
    assert q.tolist() == [2 ** 14 + 2 ** 15, 2 ** 15 + s, 2 ** 14 + s, -1, -1]
    st = KT.statistics(q, 1.0)
    vals = [int(v) for v in q[:3]]
    mu = sum(vals) / 3
    sd = math.sqrt(sum((v - mu) ** 2 for v in vals) / 2)
    assert st["n"] == 3 and st["S1"] == sum(vals) and st["S2"] == sum(v * v for v in vals)
    assert abs(st["T"] - (mu + sd)) <= 1e-9 * st["T"] and st["kept"].tolist() == [0, 2]
    assert cloud.statistical_threshold(st["n"], st["S1"], st["S2"], 1.0) == st["T"]
    assert cloud.statistical_threshold(1, 7, 49, 3.0) == 7.0 and cloud.statistical_threshold(0, 0, 0, 3.0) < 0      # n < 2
    one = KT.statistics(np.array([-1, 12, -1], np.int32), 2.0)
    assert one["T"] == 12.0 and one["kept"].tolist() == [1]
    assert len(KT.statistics(np.array([-1, -1], np.int32), 2.0)["kept"]) == 0
    big = 2 ** 22                                                               # S2 beyond 64 bits stays exact in Python
    assert cloud.statistical_threshold(2 ** 30, big * 2 ** 30, big * big * 2 ** 30, 2.0) == float(big)


def test_moments_of_the_k_nearest_are_the_radius_moments_when_k_covers():
    p, r = CT.lattice()
    want = CT.neighbors(p, r)
    assert want["count"].max() - 1 <= 8
    count, mom = KT.moments(p, r, KT.knn(KT.ranked(p, r), 8))
    assert count.tobytes() == want["count"].tobytes() and mom.tobytes() == want["moments"].tobytes()


# ---- host checks -----------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_the_library_is_needed(monkeypatch):
    p = torch.from_numpy(CT.plane()[0])
    c = torch.zeros((len(p), 3), dtype=torch.uint8)
    idx = torch.arange(len(p))
    monkeypatch.setattr(_ffi, "lib", lambda: pytest.fail("the library was loaded"))
    nan, inf = float("nan"), float("inf")
    for k in (0, 65, -1, True, False, 8.0, 2.5, None, "8", 2 ** 40):
        with pytest.raises(ValueError, match="k must be"):
            cloud.cloud_knn(p, k, 0.05)
        with pytest.raises(ValueError, match="k must be"):
            cloud.remove_statistical_outliers(p, c, k=k, radius=0.05)
        with pytest.raises(ValueError, match="k must be"):
            cloud.cloud_normals_knn(p, 0.05, k)
    for r in (0.0, -1.0, nan, inf, 1e-60, None, "1", True):
        with pytest.raises(ValueError):
            cloud.cloud_knn(p, 8, r)
        with pytest.raises(ValueError):
            cloud.remove_statistical_outliers(p, c, radius=r)
        with pytest.raises(ValueError):
            cloud.cloud_normals_knn(p, r, 8)
    for bad in (p.double(), p.reshape(-1), p[:, :2], p.numpy(), torch.empty((4, 3), device="meta")):
        with pytest.raises(ValueError, match="queries"):
            cloud.cloud_knn(p, 8, 0.05, queries=bad)
    for bad in (p.double(), p.reshape(-1), p.numpy(), None):
        with pytest.raises(ValueError):
            cloud.cloud_knn(bad, 8, 0.05)
    for ratio in (nan, inf, -inf, None, "2", True):
        with pytest.raises(ValueError, match="std_ratio"):
            cloud.remove_statistical_outliers(p, c, radius=0.05, std_ratio=ratio)
    for args, kw in (((p, c[:-1]), {}), ((p, None), {}), ((p, c, idx[:-1]), {}), (((p, c), c), {}), (((p,),), {}),
                     ((p, c), dict(radius=None))):
        with pytest.raises(ValueError):
            cloud.remove_statistical_outliers(*args, **{"radius": 0.05, **kw})
    for kw in (dict(min_points=0), dict(toward=torch.zeros(4))):
        with pytest.raises(ValueError):
            cloud.cloud_normals_knn(p, 0.05, 8, **kw)
    for call in (lambda: cloud.cloud_knn(p, 8, 0.05), lambda: cloud.cloud_knn(p, 8, 0.05, queries=p[:5]),
                 lambda: cloud.remove_statistical_outliers((p, c, idx), radius=0.05),
                 lambda: cloud.cloud_normals_knn((p, c), 0.05, 16, toward=torch.zeros(3))):
        with pytest.raises(RuntimeError, match="ROCm device"):
            call()


def test_re_exports_and_signatures():
    for n in ("cloud_knn", "KnnResult", "remove_statistical_outliers", "cloud_normals_knn"):
        assert n in mast3r_utils.__all__ and n in cloud.__all__ and getattr(mast3r_utils, n) is getattr(cloud, n)
    E = inspect.Parameter.empty
    sig = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    assert sig(cloud.cloud_knn) == [("points", E), ("k", E), ("radius", E), ("queries", None), ("workspace", None)]
    assert sig(cloud.remove_statistical_outliers) == [("points", E), ("colors", None), ("index", None), ("k", 20), ("std_ratio", 2.0),
                                                      ("radius", None), ("return_rows", False), ("return_stats", False)]
    assert sig(cloud.cloud_normals_knn) == [("points", E), ("radius", E), ("k", E), ("toward", None), ("min_points", 3),
                                            ("return_variation", False), ("workspace", None), ("return_moments", False)]
    assert cloud.KnnResult._fields == ("index", "dist2", "found", "out_of_range") and cloud.MAX_K == KT.MAX_K == 64
    for fn in (cloud.cloud_knn, cloud.remove_statistical_outliers):
        assert "ordered by row" in fn.__doc__ or "Open3D" in fn.__doc__
    assert "dropped" in cloud.cloud_knn.__doc__ and "radius bound" in cloud.remove_statistical_outliers.__doc__


# ---- the C entry points ----------------------------------------------------------------------------------------------
def test_symbols_launches_and_argument_validation(built_lib):
    names = [n for n in _ffi.declared_symbols() if n.startswith("m3_knn_")]
    assert sorted(names) == ["m3_knn_launches", "m3_knn_mean_distance", "m3_knn_moments", "m3_knn_query", "m3_knn_stat_count",
                             "m3_knn_stat_scatter"]
    for n in names:
        assert hasattr(built_lib, n), n
    L = _ffi.lib()
    assert L.m3_knn_launches() == 7 == L.m3_cloud_launches()
    for n in names:
        getattr(built_lib, n).argtypes, getattr(built_lib, n).restype = getattr(L, n).argtypes, getattr(L, n).restype
    one, big = 0x1000, 1 << 40                                                  # never dereferenced: every call below is refused
    nan, inf = float("nan"), float("inf")
    short = L.m3_cloud_ws_bytes(8) - 1
    qy = lambda **k: built_lib.m3_knn_query(*[k.get(n, d) for n, d in (
        ("points", one), ("M", 8), ("radius", 0.5), ("queries", None), ("Q", 8), ("k", 4), ("index", one), ("dist2", one),
        ("found", one), ("ws", one), ("ws_bytes", big), ("stream", None))])
    for bad in (dict(points=None), dict(index=None), dict(dist2=None), dict(found=None), dict(ws=None), dict(M=-1),
                dict(M=2 ** 30 + 1), dict(Q=7), dict(Q=-1, queries=one), dict(Q=2 ** 30 + 1, queries=one), dict(k=0), dict(k=65),
                dict(k=-1), dict(radius=0.0), dict(radius=nan), dict(radius=inf), dict(ws=one + 8), dict(ws_bytes=short),
                dict(points=one + 2), dict(queries=one + 2), dict(index=one + 2), dict(dist2=one + 1), dict(found=one + 2)):
        assert qy(**bad) == -1, bad
    mo = lambda **k: built_lib.m3_knn_moments(*[k.get(n, d) for n, d in (
        ("points", one), ("M", 8), ("radius", 0.5), ("scale", 2.0 ** 21), ("index", one), ("found", one), ("k", 4), ("count", one),
        ("moments", one), ("stream", None))])
    for bad in (dict(points=None), dict(index=None), dict(found=None), dict(count=None), dict(moments=None), dict(M=-1), dict(k=0),
                dict(k=65), dict(radius=nan), dict(scale=0.0), dict(scale=2.0 ** 23), dict(scale=inf), dict(moments=one + 4),
                dict(index=one + 2)):
        assert mo(**bad) == -1, bad
    md = lambda **k: built_lib.m3_knn_mean_distance(*[k.get(n, d) for n, d in (
        ("points", one), ("M", 8), ("factor", 2.0 ** 34), ("index", one), ("found", one), ("k", 4), ("q", one), ("ws", one),
        ("ws_bytes", big), ("stream", None))])
    for bad in (dict(points=None), dict(index=None), dict(found=None), dict(q=None), dict(ws=None), dict(M=-1), dict(k=0), dict(k=65),
                dict(factor=0.0), dict(factor=nan), dict(factor=inf), dict(ws=one + 4), dict(ws_bytes=short), dict(q=one + 2)):
        assert md(**bad) == -1, bad
    sc = lambda **k: built_lib.m3_knn_stat_count(*[k.get(n, d) for n, d in (
        ("q", one), ("M", 8), ("threshold", 2), ("ws", one), ("ws_bytes", big), ("stream", None))])
    for bad in (dict(q=None), dict(ws=None), dict(M=-1), dict(threshold=-1), dict(ws=one + 4), dict(ws_bytes=short), dict(q=one + 2)):
        assert sc(**bad) == -1, bad
    ss = lambda **k: built_lib.m3_knn_stat_scatter(*[k.get(n, d) for n, d in (
        ("points", one), ("colors", one), ("index", one), ("q", one), ("M", 8), ("threshold", 2), ("ws", one), ("ws_bytes", big),
        ("M2", 4), ("points_out", one), ("colors_out", one), ("index_out", one), ("rows_out", one), ("stream", None))])
    for bad in (dict(points=None), dict(q=None), dict(ws=None), dict(points_out=None), dict(M=-1), dict(M2=-1), dict(M2=9),
                dict(threshold=-1), dict(ws_bytes=short), dict(colors=None), dict(colors_out=None), dict(index_out=None),
                dict(rows_out=one + 4)):
        assert ss(**bad) == -1, bad
