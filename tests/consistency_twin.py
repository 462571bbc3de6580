"""Float64 oracle of the multi-view consistency rule (csrc/consistency.hip), in numpy, the seeded
scenes its tests use, and what a device result has to satisfy.  Plain helper module: numpy only.

The rule, word for word.  Inputs: the keyframe tables (X float32 [K,N,3] in each keyframe's own camera frame, C float32
[K,N], poses float32 [K,8], N_k), the common grid H x W (N = H * W), a pinhole (fx, fy, cx, cy) of that grid, a neighbour
table nbr int32 [K,V] with -1 for "none", and the scalars thr (or None), z_min, depth_rtol, min_views, max_conflicts (or
None).

    1. observation plane   D[j][m] = X_j[m].z when point (j, m) passes the exporter's confidence test (C / N_j > thr:
                           fp32 divide, strict, NaN fails; thr None: no test), X_j[m].z is finite and X_j[m].z > z_min;
                           otherwise NaN.  X is already in j's camera frame: this is j's observed depth at pixel m.
    2. source candidates   (k, n) is a candidate exactly when the exporter would keep it: the confidence test and a
                           finite world point p = act(T_k, X).  A non-candidate has support = conflict = 0 and is not
                           kept.
    3. counting            for each slot v of nbr[k]: j = nbr[k][v]; skip when j < 0, j >= K or j == k.
                           c = (R_j^T (p - t_j)) * (1 / s_j) by the renderer's view-inverse formula (render_twin.
                           view_inverse: nine entries, t, 1 / s formed in float64 and rounded to fp32; then separately
                           rounded operations).  Skip unless c.z > z_min (strict, NaN fails).
                           u = fx * (c.x / c.z) + cx, v likewise; px = floor(u + 0.5), py likewise.  Skip unless
                           0 <= px < W and 0 <= py < H.  d = D[j][py * W + px]; NaN: j has no observation there, skip.
                           |c.z - d| <= depth_rtol * d: support += 1.  Else c.z < d: conflict += 1 (the point floats in
                           front of the surface j saw along that pixel: j saw through it).  Else nothing: occluded in j.
    4. keeping             kept = candidate and support >= min_views and (max_conflicts is None or conflict <=
                           max_conflicts).
    5. outputs             support uint8 [K,N], conflict uint8 [K,N], conf float32 [K,N] = C[k][n] when kept, else -inf.

The device rounds every step to fp32, so the twin also marks the pairs (k, n, j) that fp32 cannot decide:

    contested pair     c.z within a relative Z_EDGE = 1e-4 of z_min; or u + 0.5 or v + 0.5 within PIX_EPS = 1e-3 of an
                       integer while the point is within one pixel of the image; or
                       | |c.z - d| - depth_rtol * d | <= D_EDGE * d with D_EDGE = 1e-4
    contested source   any of its pairs is contested

check_against_twin: on uncontested sources support, conflict and the bytes of conf are exact; on a contested source each
count lies within the number of its contested pairs of the twin's and conf is C or -inf.  A scene with more than 5 %
contested candidates fails as untestable (the renderer's cap: a condition, not a measurement).  fp32_emulation is the
same rule in numpy float32 (not the device's bits: numpy does not promise the device's operation order inside act).
"""
import numpy as np

import render_scenes as RS
import render_twin as RT
from oracle import sim3 as S

PIX_EPS, Z_EDGE, D_EDGE, MAX_CONTESTED = 1e-3, 1e-4, 1e-4, 0.05
FLT_MAX = RT.FLT_MAX


def all_others(K):
    """nbr [K, K-1]: every other keyframe, ascending (neighbours=None)."""
    j = np.arange(K - 1)[None, :]
    return (j + (j >= np.arange(K)[:, None])).astype(np.int32)


def nearest(T, V):
    """nbr [K, min(V, K-1)] of neighbours=V: fp32 squared centre distances, diagonal +inf, stable argsort."""
    t = np.asarray(T, dtype=np.float32)[:, :3]
    d = t[:, None, :] - t[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    np.fill_diagonal(d2, np.inf)
    return np.argsort(d2, axis=1, kind="stable")[:, :max(0, min(V, t.shape[0] - 1))].astype(np.int32)


def twin(sc, pinhole, nbr, thr=1.5, z_min=1e-3, depth_rtol=0.03, min_views=2, max_conflicts=1, dtype=np.float64):
    """sc: dict X float32 [K,N,3], C float32 [K,N], Nk int [K], T float32 [K,8], H, W.  Returns a dict: support, conflict
    (int64 [K,N]), kept, cand (bool [K,N]), conf float32 [K,N], pairs (int64 [K,N]: contested pairs per source)."""
    f = dtype
    Kf, N = sc["X"].shape[:2]
    H, W = sc["H"], sc["W"]
    assert H * W == N
    nbr = np.asarray(nbr, dtype=np.int64).reshape(Kf, -1)
    zmin, rtol = f(np.float32(z_min)), f(np.float32(depth_rtol))
    fx, fy, cx, cy = (f(np.float32(v)) for v in pinhole)
    with np.errstate(all="ignore"):
        avg = sc["C"].astype(np.float32) / sc["Nk"].astype(np.float32)[:, None]
        passes = np.ones((Kf, N), dtype=bool) if thr is None else avg > np.float32(thr)
        z_own = sc["X"][..., 2].astype(np.float32)
        D = np.where(passes & np.isfinite(z_own) & (z_own > np.float32(z_min)), z_own, np.float32(np.nan)).astype(f)
        if dtype == np.float64:
            world = S.sim3_act_mlx(sc["T"].astype(np.float64)[:, None, :], sc["X"].astype(np.float64))
        else:
            world = S.sim3_act_mlx(sc["T"].astype(np.float32)[:, None, :], sc["X"].astype(np.float32)).astype(np.float32)
        cand = passes & np.isfinite(world).all(axis=2) & (np.abs(world) <= FLT_MAX).all(axis=2)
        support = np.zeros((Kf, N), dtype=np.int64)
        conflict = np.zeros((Kf, N), dtype=np.int64)
        pairs = np.zeros((Kf, N), dtype=np.int64)
        half = f(0.5)
        for k in range(Kf):
            for j in nbr[k]:
                if j < 0 or j >= Kf or j == k:
                    continue
                Rt, t, inv_s = RT.view_inverse(sc["T"][j], f)
                dl = world[k].astype(f) - t
                c = np.stack([((Rt[i, 0] * dl[:, 0] + Rt[i, 1] * dl[:, 1]) + Rt[i, 2] * dl[:, 2]) * inv_s for i in range(3)], axis=1)
                cz = c[:, 2]
                front = cand[k] & (cz > zmin)
                a = (fx * (c[:, 0] / cz) + cx) + half
                b = (fy * (c[:, 1] / cz) + cy) + half
                pa, pb = np.floor(a), np.floor(b)
                inside = front & (pa >= 0) & (pa < W) & (pb >= 0) & (pb < H)
                pix = np.where(inside, pb * W + pa, 0).astype(np.int64)
                d = np.where(inside, D[j][pix], f(np.nan))
                seen = inside & ~np.isnan(d)
                diff = np.abs(cz - d)
                agree = seen & (diff <= rtol * d)
                through = seen & ~agree & (cz < d)
                support[k] += agree
                conflict[k] += through
                # what fp32 cannot decide
                z_edge = cand[k] & (np.abs(cz - zmin) <= Z_EDGE * zmin)
                maybe_front = cand[k] & (cz > zmin * (1 - Z_EDGE))
                a64, b64 = a.astype(np.float64), b.astype(np.float64)
                near_image = np.isfinite(a64) & np.isfinite(b64) & (a64 > -1) & (a64 < W + 1) & (b64 > -1) & (b64 < H + 1)
                pix_edge = maybe_front & near_image & ((np.abs(a64 - np.round(a64)) < PIX_EPS) | (np.abs(b64 - np.round(b64)) < PIX_EPS))
                d_edge = seen & (np.abs(diff - rtol * d) <= D_EDGE * d)
                pairs[k] += z_edge | pix_edge | d_edge
    kept = cand & (support >= min_views) & (True if max_conflicts is None else conflict <= max_conflicts)
    conf = np.where(kept, sc["C"].astype(np.float32), np.float32(-np.inf)).astype(np.float32)
    return dict(support=support, conflict=conflict, kept=kept, cand=cand, conf=conf, pairs=pairs)


def fp32_emulation(sc, pinhole, nbr, **kw):
    """The rule in numpy float32: (support uint8, conflict uint8, conf float32) shaped like the device's outputs."""
    tw = twin(sc, pinhole, nbr, dtype=np.float32, **kw)
    return tw["support"].astype(np.uint8), tw["conflict"].astype(np.uint8), tw["conf"]


def contested_share(tw) -> float:
    """Contested candidates as a share of the candidates (the test's condition: at most 5 %)."""
    n = int(tw["cand"].sum())
    return float(((tw["pairs"] > 0) & tw["cand"]).sum()) / n if n else 0.0


def kept_from_counts(tw_or_cand, support, conflict, min_views, max_conflicts):
    cand = tw_or_cand["cand"] if isinstance(tw_or_cand, dict) else tw_or_cand
    return cand & (support >= min_views) & (True if max_conflicts is None else conflict <= max_conflicts)


def check_against_twin(tw, sc, support, conflict, conf, min_views, max_conflicts, label=""):
    """Device outputs (numpy: uint8, uint8, float32 [K,N]) against the twin, as the module docstring states."""
    Kf, N = sc["X"].shape[:2]
    assert support.shape == conflict.shape == conf.shape == (Kf, N)
    assert support.dtype == np.uint8 and conflict.dtype == np.uint8 and conf.dtype == np.float32
    share = contested_share(tw)
    print(f"{label}: {int(tw['cand'].sum())} candidates of {Kf * N}, contested {100 * share:.2f} %, support 0..{int(tw['support'].max())}, "
          f"conflict 0..{int(tw['conflict'].max())}, kept {int(tw['kept'].sum())}")
    assert share <= MAX_CONTESTED, f"scene is untestable: {100 * share:.2f} % of the candidates are contested"
    free = tw["pairs"] == 0
    assert np.array_equal(support[free], tw["support"][free])
    assert np.array_equal(conflict[free], tw["conflict"][free])
    assert conf[free].tobytes() == tw["conf"][free].tobytes()
    con = ~free
    assert (np.abs(support[con].astype(np.int64) - tw["support"][con]) <= tw["pairs"][con]).all()
    assert (np.abs(conflict[con].astype(np.int64) - tw["conflict"][con]) <= tw["pairs"][con]).all()
    C = sc["C"].astype(np.float32)
    same = conf.view(np.uint32) == C.view(np.uint32)
    assert (same | np.isneginf(conf)).all()
    # whatever the counts of a contested source are, kept follows from them
    kept = kept_from_counts(tw, support.astype(np.int64), conflict.astype(np.int64), min_views, max_conflicts)
    want = np.where(kept, C, np.float32(-np.inf))
    assert conf.tobytes() == want.astype(np.float32).tobytes()
    return share


# ---- scenes ----------------------------------------------------------------------------------------------------------
def shared_pinhole(H, W):
    f = 0.78 * W
    return (f, f * 1.01, (W - 1) / 2 + 0.3, (H - 1) / 2 - 0.2)


def shared_scene(K, H, W, seed, layout="u8", grid_centres=False):
    """K keyframes that really see one surface: a tilted plane n . p = h intersected by each keyframe's pinhole rays
    (shared_pinhole), poses near the identity as in render_scenes.general_scene, depth noise of 0.4 %, an 8 x 8 block per
    keyframe scaled by 0.8 or 1.25 (conflicts and occlusions), confidences straddling 1.5, a few NaN / inf planted.
    grid_centres: camera centres on a grid of 1/8 (integers over 8: exact fp32 squared distances, with ties) instead."""
    rng = np.random.default_rng(seed)
    N = H * W
    fx, fy, cx, cy = shared_pinhole(H, W)
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rays = np.stack([(j - cx) / fx, (i - cy) / fy, np.ones((H, W))], axis=2).reshape(N, 3)
    n, h = np.array([0.25, -0.15, 1.0]), 2.5
    X = np.empty((K, N, 3), dtype=np.float32)
    T = np.empty((K, 8), dtype=np.float32)
    for k in range(K):
        w = rng.normal(size=3) * 0.03
        q = np.concatenate([w / 2, [1.0]])
        q = q / np.linalg.norm(q)
        t = rng.integers(-2, 3, size=3) / 8.0 if grid_centres else rng.normal(size=3) * 0.1
        s = rng.uniform(0.95, 1.05)
        T[k] = np.concatenate([t, q, [s]])
        t, q, s = (T[k, :3].astype(np.float64), T[k, 3:7].astype(np.float64), float(T[k, 7]))
        depth = (h - n @ t) / (s * (rays @ RS.rot(q).T @ n))
        depth = depth * (1 + 0.004 * rng.normal(size=N))
        y0, x0 = rng.integers(0, H - 8), rng.integers(0, W - 8)
        blk = np.zeros((H, W), dtype=bool)
        blk[y0:y0 + 8, x0:x0 + 8] = True
        depth = np.where(blk.reshape(-1), depth * (0.8 if k % 2 == 0 else 1.25), depth)
        X[k] = rays * depth[:, None]
    Nk = (1 + (np.arange(K) * 7 + seed) % 4).astype(np.int32)
    C = (rng.uniform(0.5, 2.5, size=(K, N)) * Nk[:, None]).astype(np.float32)
    for k in range(K):
        m = rng.integers(0, N, size=6)
        C[k, m[0]] = np.float32(1.5) * np.float32(Nk[k])
        C[k, m[1]] = np.nan
        X[k, m[2], rng.integers(0, 3)] = np.nan
        X[k, m[3], rng.integers(0, 3)] = np.inf
        X[k, m[4], 2] = -np.inf
        C[k, m[5]] = np.inf
    return dict(X=X, C=C, Nk=Nk, T=T, img=RS._images(rng, K, N, layout), layout=layout, K=K, N=N, H=H, W=W)


EXACT_RTOL, EXACT_ZMIN = 2.0 ** -5, 0.125
EXACT_PINHOLE = (64.0, 64.0, 32.25, 16.5)                              # for H x W = 33 x 65; (col - cx), (row - cy) on a 1/4 grid


def exact_scene(seed, layout="u8"):
    """(scene, pinhole, nbr) with K = 4, H x W = 33 x 65 in which every fp32 operation of the rule is exact, so the
    float64 twin is the device's answer bit for bit (render_scenes.exact_scene's construction: rotations from the 12
    exact ones, power-of-two scales and depths, a 1/4 grid, depth_rtol = 2^-5, z_min = 1/8).

    Every pointmap is z * ((col - cx) / 64, (row - cy) / 64, 1): the keyframe's own rays.  Keyframes 0 and 1 share a
    rotation (a half turn or the identity) and have no translation, scales 1 and 2: a point of one lands on the same
    pixel of the other at c.z = z * s_k / s_j, with u exactly integral.  Depths are powers of two times 1, 33/32, 31/32
    (|c.z - d| == depth_rtol * d against a power-of-two d: agree), 17/16, 15/16 (occluded, seen through); at the two
    pixels whose ray components are powers of two the factor is one ulp past 33/32 and 31/32 (not agree).  5 % of the
    depths are negative (behind the neighbour, and no observation).  Keyframes 2 and 3 share a third-turn rotation,
    scales 1/2 and 1, and differ by a translation of 1/32 along the camera's x: the pixel moves by 2 / c.z - right by
    2, 1 or exactly 1/2 (u + 0.5 integral: the upper pixel), left out of keyframe 2 and right out of keyframe 3 (outside
    the image)."""
    rng = np.random.default_rng(seed)
    K, H, W = 4, 33, 65
    N = H * W
    fx, fy, cx, cy = EXACT_PINHOLE
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rays = np.stack([(j - cx) / fx, (i - cy) / fy, np.ones((H, W))], axis=2).reshape(N, 3)
    qa, qb = RS.Q12[rng.integers(0, 4)], RS.Q12[rng.integers(4, 12)]
    tb = rng.integers(-16, 17, size=3) / 4.0
    T = np.zeros((K, 8))
    T[0] = np.concatenate([[0, 0, 0], qa, [1.0]])
    T[1] = np.concatenate([[0, 0, 0], qa, [2.0]])
    T[2] = np.concatenate([tb, qb, [0.5]])
    T[3] = np.concatenate([tb + RS.rot(qb) @ np.array([-1 / 32, 0, 0]), qb, [1.0]])   # a point of 2 moves right in 3
    base = 2.0 ** rng.integers(0, 3, size=(K, N))                       # camera depth in the partner's units: 1, 2, 4
    z = np.empty((K, N))
    factor = np.array([1.0, 33 / 32, 31 / 32, 17 / 16, 15 / 16])[rng.integers(0, 5, size=(2, N))]
    z[0] = 2.0 * base[0] * factor[0]                                    # c.z in 1 = z / 2
    z[1] = base[1] * np.where(rng.uniform(size=N) < 0.5, 1.0, factor[1])  # c.z in 0 = 2 z; half stay powers of two
    z[2] = 2.0 * base[2]                                                # c.z in 3 = z / 2
    z[3] = base[3]                                                      # c.z in 2 = 2 z
    z = np.where(rng.uniform(size=(K, N)) < 0.05, -z, z)
    # one ulp past the boundary, where the ray components are powers of two: (row 16, col 32) and (row 17, col 32)
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))
    down = lambda v: float(np.nextafter(np.float32(v), np.float32(-np.inf)))
    ulp = {}
    for m, d, cz in ((16 * W + 32, 2.0, up(2.0 * 33 / 32)), (17 * W + 32, 4.0, down(4.0 * 31 / 32))):
        z[1, m] = d                                                     # the observation: D[1][m] = d
        z[0, m] = 2.0 * cz                                              # the source: c.z = cz in keyframe 1
        ulp[m] = (d, cz)
    X = rays[None] * z[:, :, None]
    X32 = X.astype(np.float32)
    assert np.array_equal(X32.astype(np.float64), X)
    Nk = (1 + (np.arange(K) + seed) % 4).astype(np.int32)
    avg = rng.integers(5, 11, size=(K, N)) / 4.0                        # 1.25 ... 2.5 on a 1/4 grid: 1.5 itself occurs
    for m in ulp:
        avg[:2, m] = 2.0
    C = (avg * Nk[:, None]).astype(np.float32)
    free = np.setdiff1d(np.arange(N), list(ulp))
    for k in range(K):
        n = rng.choice(free, size=3, replace=False)
        X32[k, n[0], rng.integers(0, 3)] = np.nan
        X32[k, n[1], rng.integers(0, 3)] = np.inf
        C[k, n[2]] = np.nan
    nbr = np.array([[1, -1], [-1, 0], [3, 2], [2, 7]], dtype=np.int32)  # padding, an own index, an index beyond K
    sc = dict(X=X32, C=C, Nk=Nk, T=T.astype(np.float32), img=RS._images(rng, K, N, layout), layout=layout, K=K, N=N, H=H, W=W,
              ulp=ulp)
    assert np.array_equal(sc["T"].astype(np.float64), T)
    return sc, EXACT_PINHOLE, nbr


def exact_scene_cases(sc, pinhole, nbr):
    """Counts of the cases the exact scene has to contain, from the float64 rule: boundary agreements, one-ulp misses,
    exactly half-integral projections, points behind a neighbour and points outside its image."""
    f = np.float64
    fx, fy, cx, cy = pinhole
    W, H = sc["W"], sc["H"]
    out = dict(boundary=0, ulp_miss=0, half=0, behind=0, outside=0)
    with np.errstate(all="ignore"):
        world = S.sim3_act_mlx(sc["T"].astype(f)[:, None, :], sc["X"].astype(f))
        for k in range(sc["K"]):
            for j in nbr[k]:
                if j < 0 or j >= sc["K"] or j == k:
                    continue
                Rt, t, inv_s = RT.view_inverse(sc["T"][j], f)
                c = ((world[k] - t) @ Rt.T) * inv_s
                ok = np.isfinite(c).all(axis=1)
                cz = c[:, 2]
                out["behind"] += int((ok & (cz < 0)).sum())
                a, b = fx * (c[:, 0] / cz) + cx + 0.5, fy * (c[:, 1] / cz) + cy + 0.5
                front = ok & (cz > EXACT_ZMIN)
                inside = front & (np.floor(a) >= 0) & (np.floor(a) < W) & (np.floor(b) >= 0) & (np.floor(b) < H)
                out["outside"] += int((front & ~inside).sum())
                out["half"] += int((inside & (a == np.floor(a))).sum())
                pix = np.where(inside, np.floor(b) * W + np.floor(a), 0).astype(np.int64)
                d = sc["X"][j, pix, 2].astype(f)
                out["boundary"] += int((inside & (d > 0) & (np.abs(cz - d) == EXACT_RTOL * d)).sum())
        for m, (d, cz) in sc["ulp"].items():
            out["ulp_miss"] += int(EXACT_RTOL * d < abs(cz - d) <= EXACT_RTOL * d * (1 + 1e-5))
    return out


def explicit_table(K):
    """A neighbour table with -1 padding, a row that names its own keyframe and a row of only -1."""
    nbr = np.array([[(k + 1) % K, -1, (k + 2) % K] for k in range(K)], dtype=np.int32)
    nbr[1] = [1, 0, -1]
    nbr[K - 1] = -1
    return nbr


SHARED = [(3, 33, 65, 11), (4, 64, 128, 12), (5, 33, 65, 13)]          # K, H, W, seed: the scenes of tests/test_gpu_consistency.py
RULES = [(0, None), (1, 0), (2, 1)]                                     # (min_views, max_conflicts)


def tables_of(sc):
    """The neighbour tables every shared scene is run with: (label, nbr as numpy, the `neighbours` argument)."""
    K = sc["K"]
    return [("all", all_others(K), None), ("nearest2", nearest(sc["T"], 2), 2), ("explicit", explicit_table(K), "tensor")]


def hand_case():
    """Three keyframes of 2 x 2 at the identity pose, pinhole (1, 1, 0.5, 0.5): point n of a keyframe lands on pixel n
    of every other at its own depth, so the counts can be read off the depths.  Returns (scene, pinhole, support,
    conflict) with the counts written out for thr = 1.5, depth_rtol = 0.03, every other keyframe as neighbour."""
    pin = (1.0, 1.0, 0.5, 0.5)
    rays = np.array([[-0.5, -0.5, 1], [0.5, -0.5, 1], [-0.5, 0.5, 1], [0.5, 0.5, 1]])
    z = np.array([[2.0, 2.0, 2.0, 2.0], [2.0, 2.05, 1.0, 4.0], [2.05, 3.0, 1.0, 2.0]])
    X = (rays[None] * z[:, :, None]).astype(np.float32)
    C = np.full((3, 4), 2.0, dtype=np.float32)
    C[2, 3] = 1.0                                                       # below 1.5: no observation, not a candidate
    T = np.tile(np.array([0, 0, 0, 0, 0, 0, 1, 1], dtype=np.float32), (3, 1))
    sc = dict(X=X, C=C, Nk=np.ones(3, dtype=np.int32), T=T, img=np.zeros((3, 4, 3), dtype=np.uint8), layout="u8", K=3, N=4,
              H=2, W=2)
    # pixel 0: 2, 2, 2.05 agree pairwise (0.05 <= 0.03 * 2 and 0.03 * 2.05)
    # pixel 1: 2 and 2.05 agree, both float in front of keyframe 2's 3 (conflict); 3 is occluded in both
    # pixel 2: keyframe 0's 2 is occluded by the 1 of both others; the two 1s agree and float in front of the 2
    # pixel 3: 2 floats in front of keyframe 1's 4; keyframe 2 has no observation and no candidate; 4 is occluded
    support = np.array([[2, 1, 0, 0], [2, 1, 1, 0], [2, 0, 1, 0]], dtype=np.uint8)
    conflict = np.array([[0, 1, 0, 1], [0, 1, 1, 0], [0, 0, 1, 0]], dtype=np.uint8)
    return sc, pin, support, conflict
