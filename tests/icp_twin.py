"""A numpy restatement of the registration rule of include/m3slam.h (the m3_icp_* text), written from that text: the
pose, the nearest target point by brute force over all pairs (no cells - the cell edge only decides which rows are in
range), the 36 terms of a row, the two-stage pairwise tree, LDL^T, Cayley's update, the flags, the history and the
evaluation, as the device must give them byte for byte.  Scalars are Python floats and arrays float64: every operation
is an IEEE one, rounded on its own.  The scenes the registration tests share are at the end."""
import math

import numpy as np

import knn_twin as KT

SUMS, TILE, STATE_WORDS, HIST_WORDS = 36, 256, 24, 5
S_ITERS, S_DONE, S_STATUS, S_PAIRS, S_COST, S_FINITE, S_FAR, S_EVAL_PAIRS, S_EVAL_COST = 13, 14, 15, 16, 17, 18, 19, 20, 21
OK, TOO_FEW, SINGULAR = 0, 1, 2
UPPER = [(a, b) for a in range(7) for b in range(a, 7)]                         # v[0 .. 27]

# The twin's error against the known motion, max |entry| of (T M - I)[:3], measured: sheet point_to_plane 4.5e-9, box
# point_to_plane 3.2e-9, box point_to_point 1.0e-9 (Ns = 513, with_scale, converged in 4, 4 and 14 iterations).  The
# sources are the target's own points moved and rounded to float32 (2^-24 relative), so the minimum is the motion itself
# up to that rounding.  tests/test_icp_host.py asserts them with a margin of 10 x, and tests/test_gpu_slam_icp.py uses
# the same bound.
RECOVERY = {("sheet", 1): 4.5e-9, ("box", 1): 3.2e-9, ("box", 0): 1.0e-9}
MARGIN = 10.0


def identity():
    return np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1], np.float64)       # R | t | s


def pose_of(M):
    """double [13] of a 4 x 4 with s R | t: s the norm of the first column, as the host takes it."""
    M = np.asarray(M, np.float64)
    s = math.sqrt(float(M[0, 0]) ** 2 + float(M[1, 0]) ** 2 + float(M[2, 0]) ** 2)
    return np.concatenate([(M[:3, :3] / s).reshape(9), M[:3, 3], [s]])


def matrix_of(pose):
    T = np.eye(4)
    T[:3, :3] = pose[12] * pose[:9].reshape(3, 3)
    T[:3, 3] = pose[9:12]
    return T


def moved(source, pose):
    """(p float64 [N,3], q32 float32 [N,3]) of the float32 rows."""
    x = np.asarray(source, np.float32).astype(np.float64).reshape(-1, 3)
    R, t, s = pose[:9], pose[9:12], pose[12]
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.stack([s * ((R[3 * a] * x[:, 0] + R[3 * a + 1] * x[:, 1]) + R[3 * a + 2] * x[:, 2]) + t[a] for a in range(3)], axis=1)
        return p, p.astype(np.float32)


def correspond(q32, target, radius, chunk=512):
    """(j int64 [N], -1 without; finite bool [N]; far bool [N]).  The result is a function of the query alone, so equal
    queries are searched once."""
    q32 = np.ascontiguousarray(q32, np.float32).reshape(-1, 3)
    target = np.ascontiguousarray(target, np.float32).reshape(-1, 3)
    r = KT.radius32(radius)
    fin, far = KT.in_range(q32, radius)
    tfin, tfar = KT.in_range(target, radius)
    rows = np.flatnonzero(tfin & ~tfar)
    P = target[rows].astype(np.float64)
    j = np.full(len(q32), -1, np.int64)
    live = np.flatnonzero(fin & ~far)
    if len(live) and len(rows):
        uq, inv = np.unique(q32[live].view(np.uint32).reshape(-1, 3), axis=0, return_inverse=True)
        uq = np.ascontiguousarray(uq).view(np.float32).reshape(-1, 3).astype(np.float64)
        best = np.full(len(uq), -1, np.int64)
        for a in range(0, len(uq), chunk):
            d2 = KT.squared_distances(P, uq[a:a + chunk])
            key = np.where(d2 <= r * r, KT.pack_key(d2, np.broadcast_to(rows[None, :], d2.shape)), ~np.uint64(0))
            k = key.min(axis=1)
            best[a:a + chunk] = np.where(k == ~np.uint64(0), -1, (k & KT.ROW_MASK).astype(np.int64))
        j[live] = best[np.asarray(inv).reshape(-1)]
    return j, fin, far


def terms(p, j, target, normals, mode):
    """(v float64 [N,36], contributes bool [N])."""
    n = len(p)
    v = np.zeros((n, SUMS))
    has = j >= 0
    jj = np.where(has, j, 0)
    tg = np.asarray(target, np.float32).reshape(-1, 3)
    if not len(tg):
        return v, np.zeros(n, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        e = p - tg[jj].astype(np.float64)
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        e0, e1, e2 = e[:, 0], e[:, 1], e[:, 2]
        one, zero = np.ones(n), np.zeros(n)
        if mode == 0:
            adds = has
            cols = [one, zero, zero, zero, z, -y, x,
                    one, zero, -z, zero, x, y,
                    one, y, -x, zero, z,
                    y * y + z * z, -(x * y), -(x * z), zero,
                    x * x + z * z, -(y * z), zero,
                    x * x + y * y, zero,
                    (x * x + y * y) + z * z,
                    e0, e1, e2, y * e2 - z * e1, z * e0 - x * e2, x * e1 - y * e0, (x * e0 + y * e1) + z * e2,
                    (e0 * e0 + e1 * e1) + e2 * e2]
        else:
            f = np.asarray(normals, np.float32).reshape(-1, 3)[jj]
            adds = has & np.isfinite(f).all(axis=1) & (f != 0).any(axis=1)
            nn = f.astype(np.float64)
            n0, n1, n2 = nn[:, 0], nn[:, 1], nn[:, 2]
            J = [n0, n1, n2, y * n2 - z * n1, z * n0 - x * n2, x * n1 - y * n0, (n0 * x + n1 * y) + n2 * z]
            rho = (n0 * e0 + n1 * e1) + n2 * e2
            cols = [J[a] * J[b] for a, b in UPPER] + [J[a] * rho for a in range(7)] + [rho * rho]
        v[adds] = np.stack(cols, axis=1)[adds]
    return v, adds


def tree(x):
    """The pairwise tree over axis -2, 256 slots: x = x[0::2] + x[1::2], eight times."""
    assert x.shape[-2] == TILE
    for _ in range(8):
        x = x[..., 0::2, :] + x[..., 1::2, :]
    return x[..., 0, :]


def tile_partials(v):
    n = len(v)
    nt = max(1, -(-n // TILE))
    pad = np.zeros((nt * TILE, v.shape[1]))
    pad[:n] = v
    return tree(pad.reshape(nt, TILE, -1))


def second_stage(part):
    nt = len(part)
    rounds = -(-nt // TILE)
    pad = np.zeros((rounds * TILE, part.shape[1]))
    pad[:nt] = part
    acc = np.zeros((TILE, part.shape[1]))
    for r in range(rounds):
        acc = acc + pad[r * TILE:(r + 1) * TILE]
    return tree(acc)


def reduce(v):
    return second_stage(tile_partials(v))


def sums(source, target, radius, pose, normals=None, mode=0):
    """dict(count int64 [3] = pairs, finite rows, rows out of range; sums float64 [36]; pairs int32 [N])."""
    p, q32 = moved(source, pose)
    j, fin, far = correspond(q32, target, radius)
    v, adds = terms(p, j, target, normals, mode)
    return dict(count=np.array([adds.sum(), fin.sum(), far.sum()], np.int64), sums=reduce(v), pairs=j.astype(np.int32), q32=q32)


def unpack(S):
    """(H [7,7] symmetric, g [7], cost) of the 36 sums."""
    H = np.zeros((7, 7))
    for k, (a, b) in enumerate(UPPER):
        H[a, b] = H[b, a] = S[k]
    return H, np.array(S[28:35], np.float64), float(S[35])


def ldl_solve(S, n):
    """delta [7] of H delta = -g on the leading n x n block, or None when a pivot fails."""
    H, g, _ = unpack(S)
    H, g = H.tolist(), g.tolist()
    L = [[0.0] * n for _ in range(n)]
    d = [0.0] * n
    for j in range(n):
        w = [0.0] * n
        piv = H[j][j]
        for k in range(j):
            w[k] = L[j][k] * d[k]
            piv = piv - L[j][k] * w[k]
        d[j] = piv
        if piv <= 1e-12 * H[j][j] or not math.isfinite(piv):
            return None
        for i in range(j + 1, n):
            a = H[j][i]
            for k in range(j):
                a = a - L[i][k] * w[k]
            L[i][j] = a / piv
    y = [0.0] * n
    for i in range(n):
        a = -g[i]
        for k in range(i):
            a = a - L[i][k] * y[k]
        y[i] = a
    delta = [0.0] * 7
    for i in range(n - 1, -1, -1):
        a = y[i] / d[i]
        for k in range(i + 1, n):
            a = a - L[k][i] * delta[k]
        delta[i] = a
    return delta


def cayley(omega):
    a0, a1, a2 = (float(w) * 0.5 for w in omega)
    c = 2.0 / (1.0 + ((a0 * a0 + a1 * a1) + a2 * a2))
    return [1.0 + c * -(a1 * a1 + a2 * a2), c * (a0 * a1 - a2), c * (a0 * a2 + a1),
            c * (a0 * a1 + a2), 1.0 + c * -(a0 * a0 + a2 * a2), c * (a1 * a2 - a0),
            c * (a0 * a2 - a1), c * (a1 * a2 + a0), 1.0 + c * -(a0 * a0 + a1 * a1)]


def update(pose, delta):
    """The pose after (tau, omega, sigma) = delta: x'' = k D x' + tau."""
    R, t, s = [float(v) for v in pose[:9]], [float(v) for v in pose[9:12]], float(pose[12])
    D = cayley(delta[3:6])
    k = 1.0 + delta[6]
    out = np.zeros(13)
    for a in range(3):
        for b in range(3):
            out[3 * a + b] = (D[3 * a] * R[b] + D[3 * a + 1] * R[3 + b]) + D[3 * a + 2] * R[6 + b]
        out[9 + a] = k * ((D[3 * a] * t[0] + D[3 * a + 1] * t[1]) + D[3 * a + 2] * t[2]) + delta[a]
    out[12] = k * s
    return out


def register(source, target, radius, normals=None, mode=0, pose=None, with_scale=False, iterations=30, tol=1e-6, min_pairs=16):
    """dict(state float64 [24], history float64 [iterations run, 5], pairs int32 [N], T [4,4])."""
    r = KT.radius32(radius)
    state = np.zeros(STATE_WORDS)
    state[:13] = identity() if pose is None else pose
    hist = []
    for _ in range(iterations):
        if state[S_DONE] or state[S_STATUS]:
            break
        got = sums(source, target, radius, state[:13], normals, mode)
        pairs, cost = int(got["count"][0]), float(got["sums"][35])
        state[S_PAIRS], state[S_COST], state[S_FINITE], state[S_FAR] = pairs, cost, got["count"][1], got["count"][2]
        state[S_ITERS] += 1.0
        delta = None
        if pairs < min_pairs:
            state[S_STATUS] = TOO_FEW
        else:
            delta = ldl_solve(got["sums"], 7 if with_scale else 6)
            if delta is None:
                state[S_STATUS] = SINGULAR
        if delta is None:
            hist.append([pairs, cost, 0.0, 0.0, 0.0])
            continue
        state[:13] = update(state[:13], delta)
        tt = (delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2]
        ww = (delta[3] * delta[3] + delta[4] * delta[4]) + delta[5] * delta[5]
        sg, rr = delta[6], tol * r
        if tt <= rr * rr and ww <= tol * tol and sg * sg <= tol * tol:
            state[S_DONE] = 1.0
        hist.append([pairs, cost, tt, ww, sg])
    got = sums(source, target, radius, state[:13], None, 0)
    state[S_FINITE], state[S_FAR] = got["count"][1], got["count"][2]
    state[S_EVAL_PAIRS], state[S_EVAL_COST] = got["count"][0], got["sums"][35]
    return dict(state=state, history=np.array(hist, np.float64).reshape(-1, HIST_WORDS), pairs=got["pairs"],
                T=matrix_of(state[:13]))


def ws_bytes(ns, nt, iterations, cloud_ws_bytes):
    """The workspace formula of the header; cloud_ws_bytes = m3_cloud_ws_bytes(nt)."""
    pad16 = lambda b: (b + 15) // 16 * 16
    return pad16(cloud_ws_bytes) + 8 * STATE_WORDS + pad16(8 * HIST_WORDS * iterations) + 8 * 40 * max(1, -(-ns // TILE))


# ---- scenes: dict(target float32 [Nt,3], normals float32 [Nt,3], radius) ---------------------------------------------
def _finish(p, n, g):
    """Float32 rows in a random order, five duplicated points appended, a few normals zeroed and one made NaN."""
    order = g.permutation(len(p))
    p, n = p[order].astype(np.float32), n[order].astype(np.float32)
    p, n = np.concatenate([p, p[:5]]), np.concatenate([n, n[:5]])
    n[::50] = 0
    n[7] = np.nan
    return p, n


def sheet():
    """A bumpy sheet without symmetry, Nt = 55 * 55 + 5."""
    g = np.random.default_rng(11)
    u, w = np.meshgrid(np.linspace(-0.5, 0.5, 55), np.linspace(-0.5, 0.5, 55))
    u, w = (u + g.uniform(-0.004, 0.004, u.shape)).ravel(), (w + g.uniform(-0.004, 0.004, w.shape)).ravel()
    z = 0.08 * np.sin(3 * u + 0.5) + 0.06 * np.cos(4.3 * w) + 0.1 * u * w + 0.05 * np.exp(-((u - 0.2) ** 2 + (w + 0.1) ** 2) / 0.01)
    zu = 0.24 * np.cos(3 * u + 0.5) + 0.1 * w - 0.05 * np.exp(-((u - 0.2) ** 2 + (w + 0.1) ** 2) / 0.01) * 2 * (u - 0.2) / 0.01
    zw = -0.258 * np.sin(4.3 * w) + 0.1 * u - 0.05 * np.exp(-((u - 0.2) ** 2 + (w + 0.1) ** 2) / 0.01) * 2 * (w + 0.1) / 0.01
    n = np.stack([-zu, -zw, np.ones_like(zu)], axis=1)
    p, n = _finish(np.stack([u, w, z], axis=1), n / np.linalg.norm(n, axis=1, keepdims=True), g)
    return dict(target=p, normals=n, radius=0.08)


def box():
    """A closed box, 0.8 x 0.6 x 0.4, each face with a rounded bump of its own."""
    g = np.random.default_rng(12)
    half = np.array([0.4, 0.3, 0.2])
    pts, nrm = [], []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            a, b = [k for k in range(3) if k != axis]
            na, nb = int(half[a] * 2 / 0.025) + 1, int(half[b] * 2 / 0.025) + 1
            ua, ub = np.meshgrid(np.linspace(-half[a], half[a], na), np.linspace(-half[b], half[b], nb))
            ua, ub = ua.ravel() + g.uniform(-0.003, 0.003, ua.size), ub.ravel() + g.uniform(-0.003, 0.003, ub.size)
            ca, cb = 0.3 * half[a] * (axis + 1) / 3 * sign, -0.4 * half[b] * sign
            bump = 0.04 * (1 + 0.3 * axis) * np.exp(-((ua - ca) ** 2 + (ub - cb) ** 2) / 0.008)
            q = np.zeros((ua.size, 3))
            q[:, a], q[:, b], q[:, axis] = ua, ub, sign * (half[axis] + bump)
            m = np.zeros((ua.size, 3))
            m[:, a] = -sign * bump * -2 * (ua - ca) / 0.008
            m[:, b] = -sign * bump * -2 * (ub - cb) / 0.008
            m[:, axis] = sign
            pts.append(q)
            nrm.append(m / np.linalg.norm(m, axis=1, keepdims=True))
    p, n = _finish(np.concatenate(pts), np.concatenate(nrm), g)
    return dict(target=p, normals=n, radius=0.08)


def plane():
    """A flat plane z = 0: point to plane cannot see in-plane motion - the singular scene."""
    g = np.random.default_rng(13)
    u, w = np.meshgrid(np.linspace(-0.5, 0.5, 40), np.linspace(-0.5, 0.5, 40))
    p = np.stack([u.ravel() + g.uniform(-0.004, 0.004, u.size), w.ravel() + g.uniform(-0.004, 0.004, u.size), np.zeros(u.size)], axis=1)
    n = np.zeros_like(p)
    n[:, 2] = 1.0
    p, n = _finish(p, n, g)
    return dict(target=p, normals=n, radius=0.08)


SCENES = {"sheet": sheet, "box": box, "plane": plane}


def motion(radius, seed=5):
    """The known Sim(3) as a pose: about 5 degrees, 0.5 r, scale 1.03."""
    g = np.random.default_rng(seed)
    axis = g.normal(size=3)
    axis /= np.linalg.norm(axis)
    th = math.radians(5.0)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K
    t = g.normal(size=3)
    t *= 0.5 * radius / np.linalg.norm(t)
    return np.concatenate([R.reshape(9), t, [1.03]])


def make_source(scene, ns, seed=5, junk=True):
    """(source float32 [ns,3], M [4,4]): every (Nt // ns or 1)-th target row moved by M and rounded to float32, so the
    registration has to find inv(M).  With at least 16 rows: a NaN row, two rows far from the target, one row out of
    cell range."""
    tg, r = scene["target"], scene["radius"]
    idx = (np.arange(ns) * max(1, len(tg) // max(ns, 1))) % len(tg)
    pose = motion(r, seed)
    src = moved(tg[idx], pose)[0].astype(np.float32)
    if junk and ns >= 16:
        src[3] = np.nan
        src[5] = [30 * r, -20 * r, 10 * r]
        src[6] = [3e7 * r, 0, 0]
        src[11] = [0, 0, 25 * r]
    return src, matrix_of(pose)


def pose_error(T, M):
    """How far T M is from the identity: (max |entry| of the 3 x 4 difference)."""
    return float(np.abs((T @ M)[:3] - np.eye(4)[:3]).max())
