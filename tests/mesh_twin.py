"""numpy restatement of the mesh rule of csrc/mesh.hip (no GPU), the scenes the mesh tests share and their plants.

Inputs, as for m3_map_export_*: device tables X[k] -> float [N,3] (points in the keyframe's own camera frame),
C[k] -> float [N], img[k]; poses [K,8], Nk [K], layout M3_MAP_IMG_*; N = H * W in row-major order, H and W given.
Parameters: stride s >= 1; edge_ratio > 0 (fp32); the export's use_thresh / thresh.

Grid.  Vertices sit at pixels (gy * s, gx * s), with gy < Hg = ceil(H / s) and gx < Wg = ceil(W / s).  The source index
of a vertex is k * N + (gy * s) * W + gx * s.  Cells are (gy, gx) with gy < Hg - 1 and gx < Wg - 1.  A cell has corners
a = (gy, gx), b = (gy, gx + 1), c = (gy + 1, gx), d = (gy + 1, gx + 1).

Candidate triangles per cell.  t = 0 is (a, c, b) and t = 1 is (b, c, d), with vertices in exactly this order.  The
diagonal is always b - c.  With image x to the right, y down and z forward, both triangles are counter-clockwise seen
from the keyframe's camera.  Their normal (v1 - v0) x (v2 - v0) points back at the camera.

Vertex validity.  This is exactly the export rule: C[k][n] / (float)Nk[k] > thresh (IEEE fp32 divide, strict, NaN
fails; use_thresh = 0 skips it); and the world point s R X + t is finite, as map_points.h computes it.

Edge test.  It works on the camera-frame points X, so it does not depend on the pose or the Sim(3) scale.  It is fp32
with every operation separately rounded.  For an edge (p, q): dx = p.x - q.x and likewise for y and z, then
l2 = (dx*dx + dy*dy) + dz*dz.  For a vertex: r2 = (x*x + y*y) + z*z.  t2 = edge_ratio * edge_ratio.  The edge passes iff
l2 <= t2 * fminf(r2_p, r2_q).  The comparison is <=, and a NaN on either side fails.  No square root is taken anywhere.

Keeping.  A triangle is kept iff its three vertices are valid and its three edges pass.  A vertex is emitted iff at
least one kept triangle references it.

Outputs.  Vertices are in ascending source index.  faces holds rows of the vertex arrays, in ascending (k, gy, gx, t).
"""
import numpy as np

from oracle import sim3 as S

THR = 1.5
F32 = np.float32


def world64(sc):
    """float64 world points [K*N,3] of every source point (oracle.sim3.sim3_act_mlx, as test_gpu_map_export.py)."""
    with np.errstate(all="ignore"):
        w = S.sim3_act_mlx(sc["T"].astype(np.float64)[:, None, :], sc["X"].astype(np.float64))
    return w.reshape(-1, 3)


def colours(sc):
    """uint8 colours [K*N,3] of every source point by the export's colour rule."""
    K, N = sc["K"], sc["H"] * sc["W"]
    if sc["layout"] == "f32":
        with np.errstate(all="ignore"):
            v = np.where(np.isnan(sc["img"]), F32(0), sc["img"])
            col = np.floor(np.clip(v, F32(0), F32(1)) * F32(255)).astype(np.uint8)
        return col.transpose(0, 2, 1).reshape(K * N, 3)
    return sc["img"].reshape(K * N, 3)


def _edge(p, q, rp, rq, t2):
    d = p - q
    l2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert l2.dtype == np.float32
    return l2 <= t2 * np.fmin(rp, rq)                                          # fminf; a NaN on either side compares false


def mesh_twin(sc, thr, stride, edge_ratio):
    """(kept faces as source-index triples int64 [F,3] in order, used source indices int64 [V] ascending, candidate
    face count) of scene `sc` by the rule above."""
    K, H, W = sc["K"], sc["H"], sc["W"]
    N, s = H * W, int(stride)
    with np.errstate(all="ignore"):
        avg = sc["C"] / sc["Nk"].astype(F32)[:, None]                          # fp32 IEEE division
        valid = np.isfinite(world64(sc)).all(axis=1).reshape(K, N)
        if thr is not None:
            valid &= avg > F32(thr)
        G = sc["X"].reshape(K, H, W, 3)[:, ::s, ::s]
        Vd = valid.reshape(K, H, W)[:, ::s, ::s]
        src = (np.arange(K, dtype=np.int64)[:, None, None] * N + np.arange(H, dtype=np.int64)[None, :, None] * W
               + np.arange(W, dtype=np.int64)[None, None, :])[:, ::s, ::s]
        Hg, Wg = G.shape[1], G.shape[2]
        assert Hg == -(-H // s) and Wg == -(-W // s) and G.dtype == np.float32
        cand = 2 * K * max(Hg - 1, 0) * max(Wg - 1, 0)
        if cand == 0:
            return np.zeros((0, 3), np.int64), np.zeros((0,), np.int64), 0
        r2 = (G[..., 0] * G[..., 0] + G[..., 1] * G[..., 1]) + G[..., 2] * G[..., 2]
        t2 = F32(edge_ratio) * F32(edge_ratio)
        cut = lambda A: (A[:, :-1, :-1], A[:, :-1, 1:], A[:, 1:, :-1], A[:, 1:, 1:])
        (a, b, c, d), (ra, rb, rc, rd), (va, vb, vc, vd), (ia, ib, ic, id_) = cut(G), cut(r2), cut(Vd), cut(src)
        t0 = va & vc & vb & _edge(a, c, ra, rc, t2) & _edge(c, b, rc, rb, t2) & _edge(b, a, rb, ra, t2)
        t1 = vb & vc & vd & _edge(b, c, rb, rc, t2) & _edge(c, d, rc, rd, t2) & _edge(d, b, rd, rb, t2)
    tri = np.stack([np.stack([ia, ic, ib], axis=-1), np.stack([ib, ic, id_], axis=-1)], axis=3)     # [K,Hc,Wc,2,3]
    faces = tri[np.stack([t0, t1], axis=3)]                                    # C order: ascending (k, gy, gx, t)
    return faces, np.unique(faces), cand


def make_scene(K, H, W, seed, layout, pitch=10, block=(2, 4), blob=0.15):
    """K keyframes of an H x W pointmap seen by a pinhole with f = W: a tilted plane near z = 2 with rectangular blocks
    near z = 1 (one per `pitch` x `pitch` pixels, `block` pixels on a side: steps far above any tested edge_ratio),
    X = z * ray; smooth confidence blobs of radius about `blob` * the image size that push part of the image below THR;
    random poses, fusion counts and images as test_gpu_map_export.make_scene."""
    rng = np.random.default_rng(seed)
    N = H * W
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.stack([(u - (W - 1) / 2) / W, (v - (H - 1) / 2) / W, np.ones_like(u)], axis=-1)
    X = np.empty((K, N, 3), np.float32)
    avg = np.empty((K, N))
    for k in range(K):
        z = 2.0 + rng.uniform(-0.3, 0.3) * (u / W - 0.5) + rng.uniform(-0.3, 0.3) * (v / W - 0.5)
        for y0 in range(0, H, pitch):
            for x0 in range(0, W, pitch):
                h, w = rng.integers(block[0], block[1] + 1, size=2)
                y, x = y0 + rng.integers(0, max(1, pitch - h)), x0 + rng.integers(0, max(1, pitch - w))
                z[y:y + h, x:x + w] = 1.0 + 0.05 * (u[y:y + h, x:x + w] / W)
        X[k] = (z[..., None] * ray).reshape(N, 3).astype(np.float32)
        a = np.full((H, W), 2.2)
        for _ in range(3):
            cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), blob * rng.uniform(0.7, 1.3) * max(H, W)
            a -= 1.0 * np.exp(-((v - cy) ** 2 + (u - cx) ** 2) / (2 * r * r))
        avg[k] = a.reshape(N)
    Nk = (1 + (np.arange(K) * 7 + seed) % 4).astype(np.int32)
    C = (avg * Nk[:, None]).astype(np.float32)
    q = rng.normal(size=(K, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    T = np.concatenate([rng.normal(size=(K, 3)), q, rng.uniform(1.1, 1.3, size=(K, 1))], axis=1).astype(np.float32)
    if layout == "f32":
        img = rng.uniform(-0.2, 1.2, size=(K, 3, N)).astype(np.float32)
        special = np.array([0, 1, -0.0, np.nan, np.inf, -np.inf, 1e-8, 0.999999, 254 / 255, 1 / 255], dtype=np.float32)
        for k in range(K):
            for c in range(3):
                img[k, c, rng.integers(0, N, size=min(N, special.size))] = special[:min(N, special.size)]
    else:
        img = rng.integers(0, 256, size=(K, N, 3)).astype(np.uint8)
    return dict(X=X, C=C, Nk=Nk, T=T, img=img, layout=layout, K=K, H=H, W=W)


def _plane(H, W):
    """float32 [H*W,3]: the fronto-parallel plane z = 2 as the f = W pinhole sees it."""
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.stack([(u - (W - 1) / 2) / W, (v - (H - 1) / 2) / W, np.ones_like(u)], axis=-1)
    return (2.0 * ray).reshape(H * W, 3).astype(np.float32)


def plant(sc, rng, regions=True, empty_middle=True):
    """NaN / +inf / -inf coordinates, NaN and inf confidences, a confidence exactly at THR * N_k (strict: invalid);
    regions: in keyframe 0 ten rows with everything kept and ten with nothing kept (each more than the 8 cell rows x
    256 columns of one workgroup tile at these widths); empty_middle: with K >= 3, keyframe 1 keeps nothing."""
    K, H, W, X, C, Nk = sc["K"], sc["H"], sc["W"], sc["X"], sc["C"], sc["Nk"]
    N = H * W
    if regions and H >= 24:
        X[0, :11 * W] = _plane(H, W)[:11 * W]                                # rows 0 .. 10: a plane, confident
        C[0, :11 * W] = 2.25 * Nk[0]
        C[0, 12 * W:23 * W] = 0.25 * Nk[0]                                   # rows 12 .. 22: nothing valid
    if empty_middle and K >= 3:
        C[1] = 0.25 * Nk[1]
    if N > 8:
        for k in range(K):
            n = rng.integers(11 * W if regions and H >= 24 else 0, N, size=6)
            C[k, n[0]] = np.float32(THR) * np.float32(Nk[k])                 # 1.5 * N_k is exact, and so is the quotient
            C[k, n[1]] = np.nan
            X[k, n[2], rng.integers(0, 3)] = np.nan
            X[k, n[3], rng.integers(0, 3)] = np.inf
            X[k, n[4], rng.integers(0, 3)] = -np.inf
            C[k, n[5]] = np.inf
    return sc


def bound_scene():
    """Two keyframes of one cell, for edge_ratio = 0.5: a = (0, 0, 1) and b = (0.5, 0, 1) give l2 = 0.25 = t2 * min r2
    exactly, so the edge and with it triangle (a, c, b) is kept; in keyframe 1 b.x = nextafter(0.5, 1) and it is dropped.
    The other edges of that triangle pass with room; triangle (b, c, d) is dropped in both (d is far away)."""
    X = np.zeros((2, 4, 3), np.float32)
    for k in range(2):
        X[k] = [[0, 0, 1], [0.5, 0, 1], [0.25, 0.3, 1], [3, 3, 1]]
    X[1, 1, 0] = np.nextafter(np.float32(0.5), np.float32(1))
    T = np.array([[0, 0, 0, 0, 0, 0, 1, 1], [1, 2, 3, 0, 0, 0, 1, 1]], np.float32)
    return dict(X=X, C=np.full((2, 4), 2.0, np.float32), Nk=np.ones(2, np.int32), T=T,
                img=np.arange(24, dtype=np.uint8).reshape(2, 4, 3), layout="u8", K=2, H=2, W=2)


def one_cell_scene(layout):
    """K = 1, 2 x 2: one cell whose corner d is below the threshold, so exactly triangle (a, c, b) is kept at
    edge_ratio 0.8 (f = W = 2: a pixel step is about half the range)."""
    sc = make_scene(1, 2, 2, seed=1, layout=layout, pitch=9, block=(0, 0))
    sc["C"][0] = np.array([2.0, 2.0, 2.0, 1.0], np.float32) * sc["Nk"][0]
    return sc


def tall_scene(layout):
    """K = 1, 4100 x 5, for stride 1, edge_ratio 0.05 and THR: 4099 cell-row segments, three more than one round of the
    scan (4096 counts), at 20 500 points.  The last 8 image rows are a confident plane (as plant's rows 0 .. 10), so
    kept triangles lie in cell rows >= 4096 and a wrong carry into the second round moves their rows."""
    sc = plant(make_scene(1, 4100, 5, seed=11, layout=layout, pitch=64, blob=0.02), np.random.default_rng(111), regions=False)
    last = 8 * sc["W"]
    sc["X"][0, -last:] = _plane(sc["H"], sc["W"])[-last:]
    sc["C"][0, -last:] = 2.25 * sc["Nk"][0]
    return sc


# (name, scene arguments, plant arguments, threshold, stride, edge_ratio): every scene and parameter set the GPU tests
# use.  f = W, so a pixel step is about 1 / W of the range and the diagonal of a stride-s cell about 1.45 s / W; the
# edge ratios leave a margin of about 2x over that, far below the step between the plane and the blocks (about 1).
CASES = [
    ("33x65", dict(K=3, H=33, W=65, seed=5), {}, THR, 1, 0.05),
    ("33x65 stride 2", dict(K=3, H=33, W=65, seed=5, pitch=20, block=(4, 8)), {}, THR, 2, 0.1),
    ("33x65 stride 3", dict(K=3, H=33, W=65, seed=5, pitch=30, block=(6, 10)), {}, THR, 3, 0.15),
    ("33x65 no threshold", dict(K=3, H=33, W=65, seed=6, pitch=6, block=(2, 4)), dict(empty_middle=False), None, 1, 0.05),
    ("64x128", dict(K=2, H=64, W=128, seed=7), {}, THR, 1, 0.03),
    ("10x530", dict(K=1, H=10, W=530, seed=8), dict(regions=False), THR, 1, 0.008),
    ("10x530 stride 2", dict(K=1, H=10, W=530, seed=8, pitch=20, block=(4, 8)), dict(regions=False), THR, 2, 0.016),
    ("33x65 middle", dict(K=3, H=33, W=65, seed=9), dict(empty_middle=False), THR, 1, 0.05),
]


def case_scene(name, layout="f32"):
    for n, kw, pkw, thr, stride, ratio in CASES:
        if n == name:
            sc = plant(make_scene(layout=layout, **kw), np.random.default_rng(kw["seed"] + 100), **pkw)
            return sc, thr, stride, ratio
    raise KeyError(name)


def frames_of(sc, dev, offset=0):
    """Frames of a scene on `dev`; offset > 0: every tensor is a view that starts `offset` elements into its allocation."""
    import torch
    from mast3r_slam.frame import Frame
    K, H, W = sc["K"], sc["H"], sc["W"]
    N = H * W

    def put(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        if not offset:
            return t
        buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=dev)
        buf[offset:] = t.reshape(-1)
        return buf[offset:].view(t.shape)

    out = []
    for k in range(K):
        f = Frame(frame_id=k, img=put(sc["img"][k].reshape((3, H, W) if sc["layout"] == "f32" else (H, W, 3))),
                  T_WC=torch.from_numpy(sc["T"][k:k + 1]).to(dev))
        f.X_canon, f.C, f.N = put(sc["X"][k]), put(sc["C"][k].reshape(N, 1)), int(sc["Nk"][k])
        out.append(f)
    return out
