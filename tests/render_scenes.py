"""Seeded scenes for the renderer tests (plain helper module: numpy only, plus frames_of for the device).

exact_scene: every fp32 operation of the rule is exact, so the float64 twin is the device's answer bit for bit.  Poses
use the 12 rotations whose quaternions have components in {0, +-1} or all +-1/2 (identity, half turns about an axis,
third turns about a diagonal: axis permutations with signs), scales are powers of two, translations and the principal
point lie on a 1/4 grid, fx = fy = 64, camera depths are powers of two and projections fall on a 1/4-pixel grid.

general_scene: K keyframes, each an H x W pointmap of a smooth surface (depth 2 ... 3 plus 1 % noise) seen from a pose
near the identity (H = 1: N rays scattered over the view instead of a pixel grid), confidences straddling 1.5, a few NaN / inf planted.  Coordinates stay below about 4, so an fp32
world point is good to about 1e-6 and a projection at fx <= 1600 and z >= 1.5 to a few 1e-4 of a pixel.
"""
import numpy as np

Q12 = np.array([[0, 0, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]] +
               [[sx * .5, sy * .5, sz * .5, .5] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], dtype=np.float64)


def rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=np.float64)


def _images(rng, K, N, layout):
    if layout == "f32":
        return rng.uniform(-0.2, 1.2, size=(K, 3, N)).astype(np.float32)
    return rng.integers(0, 256, size=(K, N, 3)).astype(np.uint8)


def exact_scene(K, N, seed, layout, size=(61, 83)):
    """(scene, view pose float32 [8], (fx, fy, cx, cy)) for a view of `size`."""
    rng = np.random.default_rng(seed)
    Hv, Wv = size
    fx = fy = 64.0
    cx, cy = Wv / 2 - 0.25, Hv / 2 + 0.5
    qv, sv = Q12[rng.integers(0, 12)], 2.0 ** rng.integers(-1, 2)
    tv = rng.integers(-16, 17, size=3) / 4.0
    view = np.concatenate([tv, qv, [sv]]).astype(np.float32)
    z = 2.0 ** rng.integers(0, 3, size=(K, N))
    u = rng.integers(-6 * 4, (Wv + 6) * 4, size=(K, N)) / 4.0                   # some land outside the image
    v = rng.integers(-6 * 4, (Hv + 6) * 4, size=(K, N)) / 4.0
    z = np.where(rng.uniform(size=(K, N)) < 0.05, -z, z)                        # behind the camera
    c = np.stack([z * ((u - cx) / fx), z * ((v - cy) / fy), z], axis=2)
    p = (sv * c) @ rot(qv).T + tv
    X = np.empty((K, N, 3))
    T = np.empty((K, 8))
    for k in range(K):
        qk, sk, tk = Q12[rng.integers(0, 12)], 2.0 ** rng.integers(-1, 3), rng.integers(-16, 17, size=3) / 4.0
        T[k] = np.concatenate([tk, qk, [sk]])
        X[k] = ((p[k] - tk) @ rot(qk)) / sk
    X32 = X.astype(np.float32)
    assert np.array_equal(X32.astype(np.float64), X)
    Nk = (1 + (np.arange(K) + seed) % 4).astype(np.int32)
    avg = rng.integers(2, 11, size=(K, N)) / 4.0                                # 0.5 ... 2.5 on a 1/4 grid: 1.5 itself occurs
    C = (avg * Nk[:, None]).astype(np.float32)
    n = rng.integers(0, N, size=(K, 3))
    for k in range(K):
        X32[k, n[k, 0], rng.integers(0, 3)] = np.nan
        X32[k, n[k, 1], rng.integers(0, 3)] = np.inf
        C[k, n[k, 2]] = np.nan
    sc = dict(X=X32, C=C, Nk=Nk, T=T.astype(np.float32), img=_images(rng, K, N, layout), layout=layout, K=K, N=N)
    return sc, view, (fx, fy, cx, cy)


def general_scene(K, H, W, seed, layout):
    rng = np.random.default_rng(seed)
    N = H * W
    fk = 0.78 * W
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x, y = (j - (W - 1) / 2) / fk, (i - (H - 1) / 2) / fk
    if H == 1:                                                                  # not an image: rays scattered over the view
        x, y = rng.uniform(-0.6, 0.6, size=(1, W)), rng.uniform(-0.45, 0.45, size=(1, W))
    X = np.empty((K, N, 3), dtype=np.float32)
    T = np.empty((K, 8), dtype=np.float32)
    for k in range(K):
        ph = rng.uniform(0, 2 * np.pi, size=2)
        d = 2.5 + 0.4 * np.sin(3 * x + ph[0]) * np.cos(2.5 * y + ph[1])
        d = d * (1 + 0.01 * rng.normal(size=d.shape))
        X[k] = np.stack([x * d, y * d, d], axis=2).reshape(N, 3)
        w = rng.normal(size=3) * 0.03
        q = np.concatenate([w / 2, [1.0]])
        T[k] = np.concatenate([rng.normal(size=3) * 0.1, q / np.linalg.norm(q), [rng.uniform(0.95, 1.05)]])
    Nk = (1 + (np.arange(K) * 7 + seed) % 4).astype(np.int32)
    C = (rng.uniform(0.5, 2.5, size=(K, N)) * Nk[:, None]).astype(np.float32)
    for k in range(K):
        n = rng.integers(0, N, size=6)
        C[k, n[0]] = np.float32(1.5) * np.float32(Nk[k])
        C[k, n[1]] = np.nan
        X[k, n[2], rng.integers(0, 3)] = np.nan
        X[k, n[3], rng.integers(0, 3)] = np.inf
        X[k, n[4], rng.integers(0, 3)] = -np.inf
        C[k, n[5]] = np.inf
    return dict(X=X, C=C, Nk=Nk, T=T, img=_images(rng, K, N, layout), layout=layout, K=K, N=N, H=H, W=W)


def general_view(size, where, seed=0):
    """(view pose float32 [8], intrinsics) for a general scene: "inside" stands among the keyframe cameras, "back" half a
    unit behind them (the map fills less of the image: more sources per covered pixel)."""
    rng = np.random.default_rng(1000 + seed)
    Hv, Wv = size
    w = rng.normal(size=3) * 0.02
    q = np.concatenate([w / 2, [1.0]])
    t = rng.normal(size=3) * 0.05 + (np.array([0, 0, -0.5]) if where == "back" else 0)
    view = np.concatenate([t, q / np.linalg.norm(q), [1.0]]).astype(np.float32)
    f = 0.78 * Wv
    return view, (f, f * 1.01, (Wv - 1) / 2 + 0.3, (Hv - 1) / 2 - 0.2)


def frames_of(sc, dev, shape=None):
    """Frame objects of a scene on `dev` (images float32 [3,H,W] or uint8 [H,W,3])."""
    import torch
    from mast3r_slam.frame import Frame
    K, N = sc["K"], sc["N"]
    H, W = shape or ((sc["H"], sc["W"]) if "H" in sc else (1, N))
    out = []
    for k in range(K):
        img = torch.from_numpy(sc["img"][k].reshape((3, H, W) if sc["layout"] == "f32" else (H, W, 3))).to(dev)
        f = Frame(frame_id=k, img=img, T_WC=torch.from_numpy(sc["T"][k:k + 1]).to(dev))
        f.X_canon, f.C, f.N = torch.from_numpy(sc["X"][k]).to(dev), torch.from_numpy(sc["C"][k].reshape(N, 1)).to(dev), int(sc["Nk"][k])
        out.append(f)
    return out
