"""Row-isolated Gauss-Newton systems for the tracking and calibrated accumulators (no GPU, no test functions).

The accumulators weigh their residual rows by run-time sigmas.  At the default sigmas one row class outweighs the other
by six or seven orders of magnitude, so the light row sits below every aggregate tolerance.  The configurations below
move the sigmas until ONE row class carries the system (and its Huber branch is in a chosen regime); the float64
oracle (oracle.tracking, oracle.gn_rays) is then the reference for exactly that row's arithmetic.

  systems        float64 (or float32: the twin) H, g, cost of one linearisation, through ot.solve_step
  twin_error     the float32 twin's error against float64 - the yardstick of the device bounds
  clear_margins  validity without the points whose branch or gate could fall differently in float32
  RAY / CALIB / BLOCKS   the configurations by name
  one_hot_positions      the points at which a group or row slip shows
"""
import numpy as np

from mast3r_slam import synthetic
from oracle import gn_rays as og
from oracle import sim3 as S
from oracle import tracking as ot

HUBER = 1.345
FLOOR_TRACK = 2e-5        # the project's bound for the tracking sums (test_normal_equations_match_oracle)
FLOOR_BLOCKS = 1e-4       # ... for the calibrated backend blocks (test_edge_blocks_every_mode_every_load_path)
TWIN_FACTOR = 4.0         # 1-ulp v_rcp_f32 / v_sqrt_f32, four points added in float32, another summation order
# tau is not used here; a regulariser of this size keeps solve_step's 7x7 solve regular for one-point (rank <= 4) systems
_REG = 1e30

# ---- the configurations, by name ---------------------------------------------------------------------------------
# regime: (row class the condition is about, lowest and highest share of its weighted residuals above k, share allowed
# on the other row class); target: the row class that must carry >= 99 % of max|H|, max|g| and the cost (None: only reported)
RAY = {
    "default":          dict(sigma_ray=0.003, sigma_dist=10.0, target=None, regime=None),
    "dist_outlier":     dict(sigma_ray=1e3, sigma_dist=1e-3, target="dist", regime=("dist", 0.9, 1.0, 0.0)),
    "dist_inlier":      dict(sigma_ray=1e3, sigma_dist=0.1, target="dist", regime=("dist", 0.0, 0.0, 0.0)),
    "dist_mixed":       dict(sigma_ray=1e3, sigma_dist=0.02, target="dist", regime=("dist", 0.3, 0.7, 0.0)),
    "ray_inlier_mixed": dict(sigma_ray=0.05, sigma_dist=1e6, target="ray", regime=("ray", 0.3, 0.7, 0.0)),
}
CALIB_GATES = dict(pixel_border=3, depth_eps=1.8)
CALIB = {
    "default":       dict(sigma_pixel=1.0, sigma_depth=10.0, target=None, regime=None),
    "depth_outlier": dict(sigma_pixel=1e6, sigma_depth=1e-3, target="depth", regime=("depth", 0.9, 1.0, 0.0)),
    "depth_inlier":  dict(sigma_pixel=1e6, sigma_depth=0.2, target="depth", regime=("depth", 0.0, 0.0, 0.0)),
    "depth_mixed":   dict(sigma_pixel=1e6, sigma_depth=0.02, target="depth", regime=("depth", 0.3, 0.7, 0.0)),
    "pixel_inlier":  dict(sigma_pixel=20.0, sigma_depth=1e6, target="pixel", regime=("pixel", 0.0, 0.0, 0.0)),
}
BLOCKS = {       # backend calibrated blocks: pixel sigma 1e4, the depth sigma small / large enough
    "depth_outlier": dict(sigma_pixel=1e4, sigma_depth=1e-4, regime=(0.9, 1.0)),
    "depth_inlier":  dict(sigma_pixel=1e4, sigma_depth=0.1, regime=(0.0, 0.0)),
}
ROWS = {"ray": {"ray": (0, 1, 2), "dist": (3,)}, "calib": {"pixel": (0, 1), "depth": (2,)}}
LOW_ROW = {"ray": "dist", "calib": "depth"}         # the row class below the aggregate tolerance at the default sigmas
CONFIGS = {"ray": RAY, "calib": CALIB}
# the shapes of the full-map comparison: the four-point loop, the calibrated one-point loop (W % 4 != 0), odd N
SHAPES = [(48, 64), (48, 62), (33, 47)]
# one-hot maps: group loop and one-point loop.  Their intrinsics (focal 0.45 W) shrink the image of the map to its middle, so that
# the corner groups project inside the gates (and every point keeps a pixel residual of up to ~3 px)
ONE_HOT_SHAPES = [(8, 12), (5, 7)]
ONE_HOT_GATES = dict(pixel_border=0.5, depth_eps=1.0)
ONE_HOT_CONFIGS = {"ray": ("default", "dist_inlier", "dist_outlier"), "calib": ("default", "depth_inlier", "depth_outlier", "pixel_inlier")}


def cfg_of(model, name, **gates):
    c = {k: v for k, v in CONFIGS[model][name].items() if k.startswith("sigma")}
    if model == "calib":
        c.update(CALIB_GATES)
    c.update(gates)
    return c


# ---- problems and poses ------------------------------------------------------------------------------------------
_cache = {}


def problem(model, h, w, one_hot=False):
    """synthetic.tracking_problem at the seeds of test_normal_equations_match_oracle (1) and
    test_calibrated_tracking_matches_oracle (8, with that test's K), Xf gathered."""
    key = (model, h, w, one_hot)
    if key not in _cache:
        pr = synthetic.tracking_problem(h, w, seed=1 if model == "ray" else 8)
        pr["Xf"] = pr["Xf_canon"][pr["idx"]]
        if model == "calib":
            pr["size"] = (h, w)
            if one_hot:
                pr["K"] = np.array([[0.45 * w, 0, (w - 1) / 2], [0, 0.45 * w, (h - 1) / 2], [0, 0, 1]], dtype=np.float32)
            else:
                pr["K"] = np.array([[float(w), 0, w / 2], [0, float(w), h / 2], [0, 0, 1]], dtype=np.float32)
        _cache[key] = pr
    return _cache[key]


def check_pose():
    """The relative pose of tests/test_gpu_tracking.py::_check_normal_equations."""
    rng = np.random.default_rng(0)
    q = np.array([0.01, -0.02, 0.015, 1.0]); q /= np.linalg.norm(q)
    return np.concatenate([rng.normal(size=3) * 0.02, q, [1.01]]).astype(np.float32)


def one_hot_pose():
    """The pose of the one-hot maps: unit scale against the problem's 1.02, so that the distance and log-depth residuals
    are ~0.02 of the depth at EVERY point (at the check pose they cross zero inside the 5x7 map, and a residual of 1e-4
    is all cancellation in float32)."""
    q = np.array([0.004, -0.006, 0.005, 1.0]); q /= np.linalg.norm(q)
    return np.concatenate([[0.012, -0.008, 0.004], q, [1.0]]).astype(np.float32)


def poses(model):
    """Ray-distance: the check pose.  Calibrated: that pose and one that shifts the projection the other way (the frame
    points of tracking_problem sit 1.6 px towards low u; this one moves them 3.5 px towards high u, and its scale of 1.04
    lifts p.z over zk), so that all four border gates fire and each depth gate rejects points the other one passes."""
    if model == "ray":
        return {"check": check_pose()}
    q = np.array([-0.01, 0.005, -0.01, 1.0]); q /= np.linalg.norm(q)
    return {"check": check_pose(), "other": np.concatenate([[0.16, 0.04, 0.0], q, [1.04]]).astype(np.float32)}


# ---- the chain, in either precision ------------------------------------------------------------------------------
def _chain(model, pr, T, cfg, valid, f):
    """(sqrt_info, r, J, extras) exactly as opt_pose_ray_dist_sim3 / opt_pose_calib_sim3 form them, on arrays of dtype f."""
    Xf = np.asarray(pr["Xf"], dtype=f).reshape(-1, 3)
    Xk = np.asarray(pr["Xk"], dtype=f).reshape(-1, 3)
    sq = np.sqrt(np.asarray(pr["Qk"], dtype=f).reshape(-1, 1))
    v = np.asarray(valid).reshape(-1, 1).astype(f)
    T = np.asarray(T, dtype=f).reshape(8)
    p, dT = ot.act_sim3(T, Xf, jacobian=True)
    if model == "ray":
        si = np.concatenate([np.repeat(f(1.0 / cfg["sigma_ray"]) * v * sq, 3, 1), f(1.0 / cfg["sigma_dist"]) * v * sq], axis=1)
        rd, drd = ot.point_to_ray_dist(p, jacobian=True)
        return si, ot.point_to_ray_dist(Xk) - rd, -drd @ dT, {}
    meas, vmeas = ot.calib_measurements(Xk, pr["size"], cfg["depth_eps"])
    si = np.concatenate([np.repeat(f(1.0 / cfg["sigma_pixel"]) * v * sq, 2, 1), f(1.0 / cfg["sigma_depth"]) * v * sq], axis=1)
    pz, dpz, vproj = ot.project_calib(p, np.asarray(pr["K"], dtype=f), pr["size"], True, cfg["pixel_border"], cfg["depth_eps"])
    si = np.where(vproj & vmeas, si, f(0.0))
    return si, meas - pz, -dpz @ dT, dict(u=pz[:, 0], v=pz[:, 1], pz=p[:, 2], zk=Xk[:, 2], gated=(vproj & vmeas)[:, 0])


def _solve(si, r, J, huber):
    _, cost, H, g = ot.solve_step(si, r, J, huber, reg=_REG)
    assert H.dtype == si.dtype and g.dtype == si.dtype                    # the float32 twin stays in float32
    return H.astype(np.float64), g.astype(np.float64), float(cost)


def systems(model, pr, T, cfg, valid=None, dtype=np.float64):
    """One linearisation at relative pose T: dict with H [7,7], g [7], cost (float64 values of a chain run in `dtype`),
    wr [N,rows] = |si * r|, the chain's si, r, J and, for the calibrated model, u, v, pz, zk and `gated` (all gates pass)."""
    valid = pr["valid"] if valid is None else valid
    si, r, J, ex = _chain(model, pr, T, cfg, valid, dtype)
    assert si.dtype == dtype and r.dtype == dtype and J.dtype == dtype
    H, g, cost = _solve(si, r, J, cfg.get("huber", HUBER))
    return dict(H=H, g=g, cost=cost, wr=np.abs(si * r), si=si, r=r, J=J, **ex)


def rows_only(model, s, cls, huber=HUBER):
    """(H, g, cost) of the row class `cls` alone (Huber weights are per row: the classes add up to the system)."""
    keep = np.zeros(s["si"].shape[1], dtype=s["si"].dtype)
    keep[list(ROWS[model][cls])] = 1
    return _solve(s["si"] * keep, s["r"], s["J"], huber)


def point_only(s, n, huber=HUBER):
    """(H, g, cost) of point n alone."""
    return _solve(s["si"][n:n + 1], s["r"][n:n + 1], s["J"][n:n + 1], huber)


def rel_err(a, b):
    """(max|dH| / max|H|, max|dg| / max|g|, |dcost| / cost) of system a against reference b (triples H, g, cost)."""
    return (np.abs(a[0] - b[0]).max() / np.abs(b[0]).max(), np.abs(a[1] - b[1]).max() / np.abs(b[1]).max(),
            abs(a[2] - b[2]) / b[2])


def twin_error(model, pr, T, cfg, valid):
    """The float32 twin's error: the same chain and solve_step on float32 arrays, against float64."""
    s64, s32 = systems(model, pr, T, cfg, valid), systems(model, pr, T, cfg, valid, np.float32)
    return rel_err((s32["H"], s32["g"], s32["cost"]), (s64["H"], s64["g"], s64["cost"]))


def bounds(twin, floor=FLOOR_TRACK):
    return tuple(max(floor, TWIN_FACTOR * e) for e in twin)


# ---- margins and gates -------------------------------------------------------------------------------------------
def gate_passes(pr, s, cfg):
    """The six gates of the calibrated model, each as `passes` [N] (float64 values of s)."""
    h, w = pr["size"]
    b, eps = cfg["pixel_border"], cfg["depth_eps"]
    return {"u_lo": s["u"] > b, "u_hi": s["u"] < w - 1 - b, "v_lo": s["v"] > b, "v_hi": s["v"] < h - 1 - b,
            "pz": s["pz"] > eps, "zk": s["zk"] > eps}


def near_decision(model, pr, s, cfg, huber=HUBER):
    """Points whose Huber branch (any row) or gate decision could differ between float32 and float64."""
    near = (np.abs(s["wr"] - huber) < 1e-3 * huber).any(axis=1)
    if model == "calib":
        h, w = pr["size"]
        b, eps = cfg["pixel_border"], cfg["depth_eps"]
        for val, edge in ((s["u"], b), (s["u"], w - 1 - b), (s["v"], b), (s["v"], h - 1 - b)):
            near |= np.abs(val - edge) < 1e-3
        near |= (np.abs(s["pz"] - eps) < 1e-5) | (np.abs(s["zk"] - eps) < 1e-5)
    return near


def clear_margins(model, pr, T, cfg, valid=None):
    """Validity for the oracle AND the device: pr's (or the given) mask without the points of near_decision.  Raises when
    that removes more than 1 % of the points that contribute."""
    valid = np.asarray(pr["valid"] if valid is None else valid).astype(bool)
    s = systems(model, pr, T, cfg, valid)
    near = near_decision(model, pr, s, cfg, cfg.get("huber", HUBER))
    contributing = valid & s["gated"] if model == "calib" else valid
    removed = int((valid & near).sum())
    if removed > 0.01 * int(contributing.sum()):
        raise ValueError(f"{removed} of {int(contributing.sum())} contributing points sit on a branch or gate margin")
    return valid & ~near


def regime_shares(model, s, valid_contrib):
    """Per row class: the share of the contributing points' weighted residuals of that class that are above k."""
    wr = s["wr"][valid_contrib]
    return {cls: float((wr[:, list(rows)] >= HUBER).mean()) if len(wr) else 0.0 for cls, rows in ROWS[model].items()}


def one_hot_positions(h, w):
    """The four lanes of the first group, the last pixel of row 0, the first of row 1, the four lanes of the last group and
    one interior point."""
    n = h * w
    return [0, 1, 2, 3, w - 1, w, n - 4, n - 3, n - 2, n - 1, (h // 2) * w + w // 2]


def one_hot(n_points, n):
    v = np.zeros(n_points, dtype=bool)
    v[n] = True
    return v


def one_hot_cfg(model, name):
    return cfg_of(model, name, **(ONE_HOT_GATES if model == "calib" else {}))


def one_hot_reference(model, h, w, name, dtype=np.float64):
    """[(n, (H, g, cost) of point n alone)] over one_hot_positions, at one_hot_pose."""
    key = ("one_hot", model, h, w, name, np.dtype(dtype).name)
    if key not in _cache:
        s = systems(model, problem(model, h, w, one_hot=True), one_hot_pose(), one_hot_cfg(model, name),
                    np.ones(h * w, dtype=bool), dtype)
        _cache[key] = [(n, point_only(s, n)) for n in one_hot_positions(h, w)]
    return _cache[key]


def one_hot_twin_error(model, h, w, name):
    """The float32 twin's error of the configuration: the largest over its one-hot points, each relative to itself."""
    e = [rel_err(b[1], a[1]) for a, b in zip(one_hot_reference(model, h, w, name), one_hot_reference(model, h, w, name, np.float32))]
    return tuple(np.max(np.array(e), axis=0))


def gate_points(name):
    """For the exact-zero check on the 48x64 calibrated problem in configuration `name`: per gate, (pose name, point) of a
    valid point that this gate alone rejects, clear of every margin."""
    out = {}
    pr, cfg = problem("calib", 48, 64), cfg_of("calib", name)
    for pn, T in poses("calib").items():
        s = systems("calib", pr, T, cfg)
        g = gate_passes(pr, s, cfg)
        ok = pr["valid"] & ~near_decision("calib", pr, s, cfg)
        for k in g:
            hit = np.where(ok & ~g[k] & np.all([g[j] for j in g if j != k], axis=0))[0]
            if k not in out and len(hit):
                out[k] = (pn, int(hit[len(hit) // 2]))
    return out


# ---- backend calibrated blocks -----------------------------------------------------------------------------------
def chain_scene(P):
    """The "chain" scene and the calibrated parameters of tests/test_gpu_gn_rays.py (its cache is shared)."""
    import test_gpu_gn_rays as G
    return G._path_scene("chain", P), G._PATH_CALIB, G._path_params(2)[1:3]


def blocks_calib(P, name):
    """(oracle calib dict, device calib tuple) of configuration `name`: _PATH_CALIB with the two sigmas replaced."""
    _, c, _ = chain_scene(P)
    sp, sd = BLOCKS[name]["sigma_pixel"], BLOCKS[name]["sigma_depth"]
    return (dict(fx=c[0], fy=c[1], cx=c[2], cy=c[3], width=c[4], height=c[5], border=c[6], z_eps=c[7], sigma_pixel=sp,
                 sigma_depth=sd), tuple(c[:8]) + (sp, sd))


def edge_block_calib(Twc, Xs, Cs, ix, jx, idx_corr, valid, q_conf, C_thresh, Q_thresh, c, dtype=np.float64, rows=(1, 1, 1)):
    """og.edge_blocks(point_mode=2) restated with the per-point arithmetic in `dtype` (the relative pose of the edge is
    formed in float64 and rounded, as the kernel does) and a row mask.  Returns (Hjj, gj, n, wr [n,3])."""
    f = dtype
    t = Twc[:, :3].astype(np.float64); q = Twc[:, 3:7].astype(np.float64); s = Twc[:, 7].astype(np.float64)
    tij, qij, sij = (np.asarray(a).astype(f) for a in S.sim3_relative(t[ix], q[ix], s[ix], t[jx], q[jx], s[jx]))
    mask = valid & (q_conf > Q_thresh) & (Cs[ix, idx_corr] > C_thresh) & (Cs[jx] > C_thresh)
    vi = np.where(mask)[0]
    Xi, Xj, conf = Xs[ix, idx_corr[vi]].astype(f), Xs[jx, vi].astype(f), q_conf[vi].astype(f)
    Y = S.quat_rotate(qij[None], Xj) * sij + tij
    keep = (Y[:, 2] > f(c["z_eps"])) & (Xi[:, 2] > f(c["z_eps"]))
    Xi, Y, conf = Xi[keep], Y[keep], conf[keep]
    one = f(1.0)
    zj, zi = one / Y[:, 2], one / Xi[:, 2]
    fx, fy, cx, cy = f(c["fx"]), f(c["fy"]), f(c["cx"]), f(c["cy"])
    pju, pjv = fx * Y[:, 0] * zj + cx, fy * Y[:, 1] * zj + cy
    piu, piv = fx * Xi[:, 0] * zi + cx, fy * Xi[:, 1] * zi + cy
    b = f(c["border"])
    inb = (pju >= b) & (pju < f(c["width"]) - b) & (pjv >= b) & (pjv < f(c["height"]) - b)
    Xi, Y, conf, zj = Xi[inb], Y[inb], conf[inb], zj[inb]
    isp, isd = f(1.0 / c["sigma_pixel"]), f(1.0 / c["sigma_depth"])
    err = np.stack([(pju[inb] - piu[inb]) * isp, (pjv[inb] - piv[inb]) * isp, (np.log(Y[:, 2]) - np.log(Xi[:, 2])) * isd], axis=-1)
    sqrt_w = np.sqrt(conf)
    n = len(Xi)
    dproj = np.zeros((n, 3, 3), dtype=f)
    dproj[:, 0, 0] = fx * zj * isp
    dproj[:, 0, 2] = -fx * Y[:, 0] * zj * zj * isp
    dproj[:, 1, 1] = fy * zj * isp
    dproj[:, 1, 2] = -fy * Y[:, 1] * zj * zj * isp
    dproj[:, 2, 2] = zj * isd
    wr = np.abs(sqrt_w[:, None] * err)
    w = S.huber_weight(sqrt_w[:, None] * err).astype(f) * (sqrt_w[:, None] ** 2) * np.asarray(rows, dtype=f)
    qi_inv = S.quat_inv(q[ix]).astype(f)
    s_inv = f(1.0 / s[ix])
    Jj = np.zeros((n, 3, 7), dtype=f)
    eye = np.eye(3, dtype=f)
    z = np.zeros(n, dtype=f)
    base_rot = np.stack([np.stack([z, Y[:, 2], -Y[:, 1]], -1), np.stack([-Y[:, 2], z, Y[:, 0]], -1),
                         np.stack([Y[:, 1], -Y[:, 0], z], -1)], axis=1)
    for k in range(3):
        Jj[:, k, :3] = s_inv * S.quat_rotate(qi_inv, eye[k])[None, :]
        Jj[:, k, 3:6] = S.quat_rotate(qi_inv[None], base_rot[:, k, :])
        Jj[:, k, 6] = Y[:, k]
    Jj = np.einsum("nrc,nck->nrk", dproj, Jj)
    wJ = w[:, :, None] * Jj
    Hjj, gj = np.einsum("nci,ncj->ij", Jj, wJ), np.einsum("nci,nc->i", wJ, err)
    assert Hjj.dtype == f and gj.dtype == f and wr.dtype == f
    return Hjj.astype(np.float64), gj.astype(np.float64), n, wr


def blocks_systems(P, name, dtype=np.float64, rows=(1, 1, 1)):
    """Every edge of the chain scene in configuration `name`: list of (Hjj, gj, n, wr)."""
    key = ("blocks", P, name, np.dtype(dtype).name, rows)
    if key not in _cache:
        (Twc, Xs, Cs, ii, jj, idx, valid, Q), _, (ct, qt) = chain_scene(P)
        oc, _ = blocks_calib(P, name)
        _cache[key] = [edge_block_calib(Twc, Xs, Cs, int(ii[e]), int(jj[e]), idx[e], valid[e], Q[e], ct, qt, oc, dtype, rows)
                       for e in range(len(ii))]
    return _cache[key]


def blocks_oracle(P, name):
    """og.edge_blocks itself on every edge: list of (Hjj, gj, n)."""
    key = ("blocks_og", P, name)
    if key not in _cache:
        (Twc, Xs, Cs, ii, jj, idx, valid, Q), _, (ct, qt) = chain_scene(P)
        oc, _ = blocks_calib(P, name)
        t = Twc[:, :3].astype(np.float64); q = Twc[:, 3:7].astype(np.float64); s = Twc[:, 7].astype(np.float64)
        _cache[key] = [og.edge_blocks(t, q, s, Xs, Cs, int(ii[e]), int(jj[e]), idx[e], valid[e], Q[e], 1.0, ct, qt, 2, oc)
                       for e in range(len(ii))]
    return _cache[key]


def blocks_twin_error(P, name):
    """Per edge (max|dH| / max|H|, max|dg| / max|g|) of the float32 restatement against float64."""
    s64, s32 = blocks_systems(P, name), blocks_systems(P, name, np.float32)
    assert all(a[2] == b[2] for a, b in zip(s64, s32))
    return [(np.abs(b[0] - a[0]).max() / np.abs(a[0]).max(), np.abs(b[1] - a[1]).max() / np.abs(a[1]).max())
            for a, b in zip(s64, s32)]


# ---- the loop that needs the distance row ------------------------------------------------------------------------
def loop_problem():
    """A 32x48 ray-distance problem between world poses whose relative pose has a translation
    (as test_nonidentity_world_poses builds them) and the dist_mixed sigmas."""
    if "loop" not in _cache:
        pr = synthetic.tracking_problem(32, 48, seed=3)
        pr["Xf"] = pr["Xf_canon"][pr["idx"]]
        rng = np.random.default_rng(5)
        qk = rng.normal(size=4); qk /= np.linalg.norm(qk)
        pr["T_WCk"] = np.concatenate([rng.normal(size=3), qk, [1.7]]).astype(np.float32)
        pr["T_WCf"] = S.sim3_mul_mlx(pr["T_WCk"].astype(np.float64), np.array([0.01, 0, 0, 0, 0, 0, 1, 1.0])).astype(np.float32)
        _cache["loop"] = pr
    return _cache["loop"]


LOOP_POSE_TOL = 5e-5      # the loop tests' bound on the relative pose (test_gn_loop_matches_oracle)
LOOP_WORLD_TOL = 2e-4     # ... on the world pose behind a keyframe pose of norm ~2 (test_nonidentity_world_poses)


def loop_twin_error(iters):
    """(t, q, s, world pose) errors of the float32 loop (ot.opt_pose_ray_dist_sim3 with dtype float32) against float64.
    It holds t and s but not q: its distance row has float32 roundoff in its rotation columns (r^T [p]x, analytically
    zero), and at sigma_ray 1e3 the rotation rests on rows 1e-10 of the system.  The device adds that row without
    rotation columns, so it is held to the loop tests' own bounds rather than to 4 x these figures."""
    a, b = loop_oracle(iters), loop_oracle(iters, np.float32)
    d = np.abs(a[1] - b[1])
    return d[:3].max(), d[3:7].max(), d[7], np.abs(a[0] - b[0]).max()


def loop_oracle(iters, dtype=np.float64):
    key = ("loop", iters, np.dtype(dtype).name)
    if key not in _cache:
        pr = loop_problem()
        cfg = {k: v for k, v in RAY["dist_mixed"].items() if k.startswith("sigma")}
        _cache[key] = ot.opt_pose_ray_dist_sim3(pr["Xf"], pr["Xk"], pr["T_WCf"], pr["T_WCk"], pr["Qk"], pr["valid"], cfg,
                                                dtype=dtype, fixed_iters=iters)
    return _cache[key]
