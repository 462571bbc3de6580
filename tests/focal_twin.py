"""Float64 restatement of the focal estimate (csrc/intrinsics.hip) in numpy, and the scene recipe of
the focal tests.

    valid(n)      <=>  C32[n] / float32(N_k) > thr (fp32 divide, strict, NaN fails; thr None: no test), x, y, z finite,
                       z > float32(z_min)
    per pixel          u = (n % W) - cx, v = (n // W) - cy, a = x / z, b = y / z, pq = a u + b v, qq = a a + b b
    f_0                sum pq / sum qq
    f_i, i = 1..iters  d = sqrt((u - f a)^2 + (v - f b)^2) at f_{i-1}, w = 1 / (d if d > 1e-8 else 1e-8),
                       sum w pq / sum w qq
    result             (f_iters, f_0, count, mean d at f_iters); no valid pixel: (NaN, NaN, 0, NaN)

Sums are numpy.sum over the valid pixels in float64: the device adds the same terms in another order.
"""
import numpy as np

D_FLOOR = 1e-8


def focal_twin(X, C, Nk, size, pp=None, thr=1.5, z_min=0.0, iters=10):
    """X float32 [N,3], C float32 [N], Nk int -> float64 [4]."""
    H, W = size
    X = np.asarray(X, dtype=np.float32).reshape(-1, 3)
    C = np.asarray(C, dtype=np.float32).reshape(-1)
    assert X.shape[0] == H * W == C.shape[0]
    cx, cy = ((W - 1) / 2.0, (H - 1) / 2.0) if pp is None else (float(pp[0]), float(pp[1]))
    with np.errstate(all="ignore"):
        ok = np.isfinite(X).all(axis=1) & (X[:, 2] > np.float32(z_min))
        if thr is not None:
            ok &= (C / np.float32(Nk)) > np.float32(thr)
    n = np.nonzero(ok)[0]
    if n.size == 0:
        return np.array([np.nan, np.nan, 0.0, np.nan])
    u, v = (n % W).astype(np.float64) - cx, (n // W).astype(np.float64) - cy
    x, y, z = (X[n, i].astype(np.float64) for i in range(3))
    with np.errstate(all="ignore"):
        a, b = x / z, y / z
        pq, qq = a * u + b * v, a * a + b * b
        f0 = f = np.float64(np.sum(pq)) / np.float64(np.sum(qq))

        def dist(f):
            du, dv = u - f * a, v - f * b
            return np.sqrt(du * du + dv * dv)

        for _ in range(iters):
            d = dist(f)
            w = 1.0 / np.where(d > D_FLOOR, d, D_FLOOR)
            f = np.float64(np.sum(w * pq)) / np.float64(np.sum(w * qq))
        return np.array([f, f0, float(n.size), np.float64(np.sum(dist(f))) / n.size])


def focal_twin_map(sc, size, **kw):
    """[K,4] of a scene dict (X [K,N,3], C [K,N], Nk [K])."""
    return np.stack([focal_twin(sc["X"][k], sc["C"][k], sc["Nk"][k], size, **kw) for k in range(sc["K"])])


def pinhole_keyframe(H, W, f, seed, out_frac=0.03, noise=0.002, nk=1):
    """(X float32 [N,3], C float32 [N]) of the recipe: a pinhole of focal f with the principal point at the image centre
    sees depth z = 2 + 0.5 sin(u / 7) + 0.3 cos(v / 5) over integer pixels (u, v); points ((u - cx) / f z, (v - cy) / f z,
    z) plus Gaussian noise of sigma `noise`; a fraction out_frac of the pixels replaced by uniform points in [-3, 3]^3
    with z <- |z| + 0.2; C uniform in [1, 3] times nk (so C / nk straddles 1.5)."""
    rng = np.random.default_rng(seed)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    z = 2.0 + 0.5 * np.sin(u / 7.0) + 0.3 * np.cos(v / 5.0)
    X = np.stack([(u - cx) / f * z, (v - cy) / f * z, z], axis=2).reshape(-1, 3)
    X = X + noise * rng.normal(size=X.shape)
    bad = rng.uniform(size=H * W) < out_frac
    wild = rng.uniform(-3.0, 3.0, size=(H * W, 3))
    wild[:, 2] = np.abs(wild[:, 2]) + 0.2
    X[bad] = wild[bad]
    C = rng.uniform(1.0, 3.0, size=H * W) * nk
    return X.astype(np.float32), C.astype(np.float32)


def pinhole_scene(H, W, focals, seed, nks=None, layout="u8", **kw):
    """Scene dict in the form of tests/render_scenes.py (frames_of turns it into Frame objects): one keyframe per entry
    of `focals`, identity poses, constant images."""
    K, N = len(focals), H * W
    nks = [1] * K if nks is None else list(nks)
    kfs = [pinhole_keyframe(H, W, f, seed + 101 * k, nk=nks[k], **kw) for k, f in enumerate(focals)]
    T = np.tile(np.array([0, 0, 0, 0, 0, 0, 1, 1], dtype=np.float32), (K, 1))
    img = np.zeros((K, N, 3), dtype=np.uint8) if layout == "u8" else np.zeros((K, 3, N), dtype=np.float32)
    return dict(X=np.stack([k[0] for k in kfs]), C=np.stack([k[1] for k in kfs]), Nk=np.asarray(nks, dtype=np.int32), T=T,
                img=img, layout=layout, K=K, N=N, H=H, W=W)
