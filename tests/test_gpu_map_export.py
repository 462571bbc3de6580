"""GPU: the map export kernels (csrc/map_export.hip) through export.collect_map, against a numpy restatement of the rule:

    kept(k, n)  <=>  C32[k][n] / float32(N_k) > thr  (strict; NaN fails; thr None: no test)  and  world point finite
    world       =    s R X + t                        (oracle.sim3.sim3_act_mlx in float64; bound 1e-5 on unit-scale data,
                                                        the bound and input family of test_track_gather_and_sim3_act)
    colour      =    float [3,H,W]: uint8(floor(clip(v, 0, 1) * float32(255))), NaN -> 0;  uint8 [H,W,3]: unchanged
    order       =    ascending k * N + n;  two calls: identical bytes
    voxel       =    per floor(p32 / float32(v)) the largest average confidence, ties to the smaller source index

Selection, colours, indices and the voxel choice are exact; only the points carry a tolerance."""
import numpy as np
import pytest
import torch

from mast3r_slam import export
from mast3r_slam.frame import Frame
from oracle import sim3 as S

pytestmark = pytest.mark.gpu
THR = 1.5


def make_scene(K, N, seed, layout, spread=1.0, conf_levels=None):
    """K keyframes of N points: X ~ N(0,1) * spread, t ~ N(0,1), scale about 1.2, fusion counts 1..4, C / N_k in
    [0.5, 2.5] straddling THR, with planted values (see plant)."""
    rng = np.random.default_rng(seed)
    X = (rng.normal(size=(K, N, 3)) * spread).astype(np.float32)
    Nk = (1 + (np.arange(K) * 7 + seed) % 4).astype(np.int32)
    avg = rng.uniform(0.5, 2.5, size=(K, N))
    if conf_levels:
        avg = np.round(avg * conf_levels) / conf_levels                       # few distinct values: many exact ties
    C = (avg * Nk[:, None]).astype(np.float32)
    q = rng.normal(size=(K, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    T = np.concatenate([rng.normal(size=(K, 3)), q, rng.uniform(1.1, 1.3, size=(K, 1))], axis=1).astype(np.float32)
    if layout == "f32":
        img = rng.uniform(-0.2, 1.2, size=(K, 3, N)).astype(np.float32)
        special = np.concatenate([np.arange(256, dtype=np.float32) / np.float32(255),
                                  np.nextafter(np.arange(256, dtype=np.float32) / np.float32(255), np.float32(-1)),
                                  np.nextafter(np.arange(256, dtype=np.float32) / np.float32(255), np.float32(2)),
                                  np.array([0, 1, -0.0, np.nan, np.inf, -np.inf, 1e-8, 0.999999], dtype=np.float32)])
        pos = rng.integers(0, N, size=(K, 3, min(N, special.size)))
        for k in range(K):
            for c in range(3):
                img[k, c, pos[k, c]] = special[:pos.shape[2]]
    else:
        img = rng.integers(0, 256, size=(K, N, 3)).astype(np.uint8)
    return dict(X=X, C=C, Nk=Nk, T=T, img=img, layout=layout, K=K, N=N)


def plant(sc, rng):
    """Points exactly at the threshold (strict: not kept), NaN / inf in X, NaN in C, an all-out and an all-in workgroup."""
    K, N, X, C, Nk = sc["K"], sc["N"], sc["X"], sc["C"], sc["Nk"]
    for k in range(K):
        n = rng.integers(0, N, size=min(N, 6))
        C[k, n[0]] = np.float32(THR) * np.float32(Nk[k])                     # 1.5 * N_k is exact, and so is the quotient
        if N > 3:
            C[k, n[1]] = np.nan
            X[k, n[2], rng.integers(0, 3)] = np.nan
            X[k, n[3], rng.integers(0, 3)] = np.inf
            X[k, n[4], rng.integers(0, 3)] = -np.inf
            C[k, n[5]] = np.inf
    if N >= 3072:
        C[0, 1024:2048] = 0.25 * Nk[0]                                        # a workgroup tile with nothing kept
        C[0, 2048:3072] = 2.25 * Nk[0]                                        # ... and one with everything kept
        X[0, 1024:3072] = np.where(np.isfinite(X[0, 1024:3072]), X[0, 1024:3072], 0)
    return sc


def frames_of(sc, dev):
    K, N = sc["K"], sc["N"]
    H, W = (128, N // 128) if N % 128 == 0 else (1, N)
    out = []
    for k in range(K):
        img = torch.from_numpy(sc["img"][k].reshape((3, H, W) if sc["layout"] == "f32" else (H, W, 3))).to(dev)
        f = Frame(frame_id=k, img=img, T_WC=torch.from_numpy(sc["T"][k:k + 1]).to(dev))
        f.X_canon, f.C, f.N = torch.from_numpy(sc["X"][k]).to(dev), torch.from_numpy(sc["C"][k].reshape(N, 1)).to(dev), int(sc["Nk"][k])
        out.append(f)
    return out


def expected(sc, thr):
    """(kept source indices, float64 world points of all K*N sources, uint8 colours of all sources, fp32 average conf)."""
    K, N = sc["K"], sc["N"]
    with np.errstate(all="ignore"):
        avg = sc["C"] / sc["Nk"].astype(np.float32)[:, None]                  # fp32 IEEE division
        world = S.sim3_act_mlx(sc["T"].astype(np.float64)[:, None, :], sc["X"].astype(np.float64))
        keep = np.isfinite(world).all(axis=2)
        if thr is not None:
            keep &= avg > np.float32(thr)
        if sc["layout"] == "f32":
            v = np.where(np.isnan(sc["img"]), np.float32(0), sc["img"])
            col = np.floor(np.clip(v, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)   # one fp32 multiply
            col = col.transpose(0, 2, 1)
        else:
            col = sc["img"]
    assert avg.dtype == np.float32
    return np.nonzero(keep.reshape(-1))[0], world.reshape(K * N, 3), col.reshape(K * N, 3), avg.reshape(-1)


def run(frames, thr, **kw):
    p, c, i = export.collect_map(frames, c_conf_threshold=thr, return_index=True, **kw)
    return p.cpu().numpy(), c.cpu().numpy(), i.cpu().numpy()


def check(sc, dev, thr):
    frames = frames_of(sc, dev)
    p, c, i = run(frames, thr)
    idx, world, col, _ = expected(sc, thr)
    assert p.shape == (idx.size, 3) and c.shape == (idx.size, 3) and i.shape == (idx.size,)
    assert p.dtype == np.float32 and c.dtype == np.uint8 and i.dtype == np.int64
    assert np.array_equal(i, idx)                                               # selection exact, in source order
    if idx.size > 1:
        assert (np.diff(i) > 0).all()
    assert np.array_equal(c, col[idx])
    err = np.abs(p - world[idx]).max() if idx.size else 0.0
    print(f"K={sc['K']} N={sc['N']} {sc['layout']} thr={thr}: kept {idx.size} of {sc['K'] * sc['N']}, max |p - p64| = {err:.3g}")
    assert err < 1e-5
    p2, c2, i2 = run(frames, thr)
    assert p.tobytes() == p2.tobytes() and c.tobytes() == c2.tobytes() and i.tobytes() == i2.tobytes()
    p3, c3 = export.collect_map(frames, c_conf_threshold=thr)                  # without the index output
    assert p3.cpu().numpy().tobytes() == p.tobytes() and c3.cpu().numpy().tobytes() == c.tobytes()
    return idx.size


SHAPES = [(1, 3), (3, 3), (1, 4999), (3, 4999), (17, 4999), (1, 128 * 256), (3, 128 * 256), (17, 128 * 256),
          (1, 512 * 512), (3, 512 * 512), (4100, 3)]                          # 4100 tiles: a second round of the scan (4096)


@pytest.mark.parametrize("layout", ["f32", "u8"])
@pytest.mark.parametrize("K,N", SHAPES)
def test_selection_points_colours_order(dev, K, N, layout):
    sc = plant(make_scene(K, N, seed=K * 31 + N % 97, layout=layout), np.random.default_rng(K + N))
    m = check(sc, dev, THR)
    if N > 100:
        assert 0.3 * K * N < m < 0.7 * K * N                                   # the threshold really splits the data
    if K * -(-N // 1024) > 4096:
        assert expected(sc, THR)[0].max() >= 4096 * N                          # kept points behind the carry of round one


@pytest.mark.parametrize("layout", ["f32", "u8"])
@pytest.mark.parametrize("K,N", [(3, 3), (3, 4999), (17, 128 * 256), (1, 512 * 512)])
def test_threshold_none_keeps_all_finite_and_inf_keeps_none(dev, K, N, layout):
    sc = plant(make_scene(K, N, seed=5 + K, layout=layout), np.random.default_rng(N))
    m = check(sc, dev, None)
    nonfinite = int((~np.isfinite(sc["X"]).all(axis=2)).sum())
    assert m == K * N - nonfinite                                               # NaN / inf confidences do not matter here
    assert check(sc, dev, float("inf")) == 0
    assert check(sc, dev, 0.0) <= m


def test_unaligned_views_take_the_scalar_path(dev):
    """X / C / image views that start 4 bytes into an allocation (no 16-byte loads possible): the result is unchanged."""
    sc = plant(make_scene(2, 4096, seed=3, layout="f32"), np.random.default_rng(1))
    frames = frames_of(sc, dev)
    ref = run(frames, THR)
    for f in frames:
        for name in ("X_canon", "C", "img"):
            t = getattr(f, name)
            buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
            buf[1:] = t.reshape(-1)
            setattr(f, name, buf[1:].view(t.shape))
            assert getattr(f, name).data_ptr() % 16 != 0
    got = run(frames, THR)
    for a, b in zip(ref, got):
        assert a.tobytes() == b.tobytes()


def thin_numpy(p32, conf, idx, v):
    """Rows of the unthinned cloud that survive: per voxel floor(p32 / float32(v)) the largest confidence, ties to the
    smaller source index; ascending."""
    key = np.floor(p32 / np.float32(v)).astype(np.int64)
    order = np.lexsort((idx, -conf.astype(np.float64)))                         # confidence descending, then index ascending
    _, first = np.unique(key[order], axis=0, return_index=True)
    return np.sort(order[first])


@pytest.mark.parametrize("layout", ["f32", "u8"])
@pytest.mark.parametrize("K,N,v", [(3, 4999, 0.25), (5, 128 * 256, 0.1), (2, 512 * 512, 0.1), (1, 3, 10.0)])
def test_voxel_thinning_is_exact(dev, K, N, v, layout):
    sc = plant(make_scene(K, N, seed=K + 11, layout=layout, spread=0.5, conf_levels=8), np.random.default_rng(N + 1))
    frames = frames_of(sc, dev)
    for thr in (THR, None):
        p, c, i = run(frames, thr)                                              # the unthinned output, checked above
        avg = expected(sc, thr)[3][i]
        if thr is None:
            ok = ~np.isnan(avg)                                                 # NaN confidences rank last by definition;
            avg = np.where(ok, avg, -np.inf)                                    # none of them ties with a planted +-inf here
        rows = thin_numpy(p, avg, i, v)
        pt, ct, it = run(frames, thr, voxel_size=v)
        print(f"K={K} N={N} v={v} thr={thr}: {i.size} -> {rows.size} voxels, {np.unique(avg).size} distinct confidences")
        if N > 100:
            assert rows.size < i.size / 2 and np.unique(avg).size < 64          # many points per voxel, many exact ties
        assert np.array_equal(it, i[rows])
        assert pt.tobytes() == p[rows].tobytes() and ct.tobytes() == c[rows].tobytes()
        pt2, ct2, it2 = run(frames, thr, voxel_size=v)
        assert pt.tobytes() == pt2.tobytes() and ct.tobytes() == ct2.tobytes() and it.tobytes() == it2.tobytes()
        pt3, ct3 = export.collect_map(frames, c_conf_threshold=thr, voxel_size=v)
        assert pt3.cpu().numpy().tobytes() == pt.tobytes() and ct3.cpu().numpy().tobytes() == ct.tobytes()


def test_voxel_key_overflow_raises(dev):
    sc = make_scene(2, 4999, seed=2, layout="u8")
    frames = frames_of(sc, dev)
    with pytest.raises(ValueError, match="voxel_size"):
        export.collect_map(frames, voxel_size=1e-7)                             # |p / v| ~ 1e7 >= 2^20
    p, c = export.collect_map(frames, voxel_size=1e-3)                          # |p / v| < 2^20 for |p| < 1000: fine
    assert 0 < p.shape[0] <= 2 * 4999
