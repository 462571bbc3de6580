"""GPU: every residual row of the Gauss-Newton accumulators against the float64 oracle, one row class at a time.

k_track_accum<RayDist>, k_track_accum<Calib> (csrc/tracking.hip) and gn_point<2> (csrc/gn_rays.hip) weigh their rows by
run-time sigmas; tests/tracking_rows.py moves them until one row class carries the system in a chosen Huber regime
(conditions asserted on the CPU in tests/test_tracking_rows_host.py).  Every comparison is held to the larger of the
project's own figure for it (2e-5 for the tracking sums, 1e-4 for the calibrated backend blocks) and 4 x the error of
the float32 twin of the same chain, computed here on the CPU.  The full-map tests also are the gate check of the
calibrated model: border 3 and depth_eps 1.8 reject a third of the map, and the sums match the oracle under that mask.

Measured on the MI355X: worst ratio over the four load paths and the poses, as H / g / cost, each relative to the
float64 max|H|, max|g| and cost.  "twin" is the float32 chain on the CPU, "bound" = max(floor, 4 x twin).

  full map (48x64 aligned and 4 bytes off, 48x62, 33x47)
  model  configuration      twin                       device                     bound
  ray    default            2.3e-7 / 1.7e-6 / 3.6e-8   5.2e-8 / 7.5e-8 / 3.7e-8   2.0e-5 / 2.0e-5 / 2.0e-5
  ray    dist_outlier       8.8e-6 / 1.7e-6 / 2.1e-6   3.7e-6 / 1.5e-6 / 3.4e-7   3.5e-5 / 2.0e-5 / 2.0e-5
  ray    dist_inlier        1.4e-7 / 2.4e-6 / 4.2e-6   5.1e-8 / 3.2e-7 / 6.6e-7   2.0e-5 / 2.0e-5 / 2.0e-5
  ray    dist_mixed         9.8e-7 / 2.2e-6 / 2.6e-6   1.3e-7 / 4.2e-7 / 3.8e-7   2.0e-5 / 2.0e-5 / 2.0e-5
  ray    ray_inlier_mixed   1.6e-7 / 1.6e-6 / 2.3e-8   1.5e-8 / 7.4e-9 / 1.2e-8   2.0e-5 / 2.0e-5 / 2.0e-5
  calib  default            3.3e-7 / 1.8e-6 / 1.2e-7   7.0e-8 / 2.2e-8 / 1.3e-8   2.0e-5 / 2.0e-5 / 2.0e-5
  calib  depth_outlier      2.0e-6 / 5.0e-6 / 4.2e-7   3.6e-6 / 3.1e-6 / 4.8e-7   2.0e-5 / 2.0e-5 / 2.0e-5
  calib  depth_inlier       9.6e-8 / 5.6e-6 / 3.3e-7   3.1e-8 / 6.8e-7 / 6.9e-7   2.0e-5 / 2.2e-5 / 2.0e-5
  calib  depth_mixed        2.1e-7 / 6.3e-6 / 8.6e-7   5.5e-8 / 1.3e-6 / 6.5e-7   2.0e-5 / 2.5e-5 / 2.0e-5
  calib  pixel_inlier       1.4e-7 / 1.2e-6 / 1.0e-7   1.0e-8 / 4.3e-8 / 5.7e-8   2.0e-5 / 2.0e-5 / 2.0e-5

  one point (worst of the eleven positions, relative to that point's own sums; 8x12 | 5x7)
  ray    default            device 2.4e-6 / 2.4e-7 / 8.3e-7 | 3.6e-6 / 2.1e-7 / 1.0e-6    bound 2.0e-5 everywhere
  ray    dist_inlier        device 3.1e-7 / 5.1e-6 / 1.0e-5 | 3.1e-7 / 2.8e-6 / 5.8e-6    bound 2.0e-5 / 2.2e-5 / 4.2e-5 | 2.0e-5 / 3.1e-5 / 6.1e-5
  ray    dist_outlier       device 5.6e-6 / 2.6e-7 / 5.1e-6 | 3.0e-6 / 1.9e-7 / 3.1e-6    bound 2.1e-5 / 2.0e-5 / 2.1e-5 | 3.0e-5 / 2.0e-5 / 3.1e-5
  calib  default            device 4.4e-7 / 1.8e-7 / 1.7e-7 | 4.2e-7 / 2.6e-7 / 2.6e-7    bound 2.0e-5 everywhere
  calib  depth_inlier       device 2.8e-7 / 4.3e-5 / 8.6e-5 | 1.3e-7 / 3.5e-6 / 7.0e-6    bound 2.0e-5 / 9.4e-5 / 1.9e-4 | 2.0e-5 / 2.0e-5 / 2.9e-5
  calib  depth_outlier      device 4.3e-5 / 2.2e-7 / 4.3e-5 | 3.6e-6 / 1.8e-7 / 3.5e-6    bound 9.4e-5 / 2.0e-5 / 9.4e-5 | 2.0e-5 everywhere
  calib  pixel_inlier       device 3.2e-7 / 2.6e-7 / 2.8e-7 | 2.9e-7 / 2.9e-7 / 4.1e-7    bound 2.0e-5 everywhere
  (the 8x12 log-depth figures are one point whose log-depth residual is 1e-3: float32 cancellation, twin 2.3e-5,
  and the kernel's __logf is about twice the twin's correctly rounded log)

  backend blocks (worst edge, H / g): depth_inlier 8.3e-9 / 6.9e-6 (P = 4100), 7.4e-9 / 5.9e-6 (4098);
  depth_outlier 8.0e-6 / 2.6e-8, 1.6e-5 / 2.4e-8; twin at most 1.3e-5 / 7.8e-6, so every bound is the 1e-4 floor.

  loop at the dist_mixed sigmas, 1 / 2 / 3 iterations: relative pose within 4.6e-8 / 4.7e-8 / 1.7e-8 of the float64 loop
  (bound 5e-5), world pose within 1.0e-7 (bound 2e-4).  The float32 numpy loop is off by 3.6e-4 ... 1.8e-3 in q.
  Before the distance row was taken out of the congruence in RayDist::point this test failed: q off by 3.8e-2 after one
  iteration, the second step refused on a negative pivot.
"""
import numpy as np
import pytest

import tracking_rows as TR
from mast3r_slam import kernels, tracker
from test_gpu_tracking import _off4, _t

pytestmark = pytest.mark.gpu

# the load paths of k_track_accum: the four-point loop; the same size 4 bytes off 16-byte alignment (one-point loop);
# W % 4 != 0 (the calibrated model's one-point loop; N % 4 == 0, so the ray-distance model stays on groups); odd N
_LAYOUTS = {"aligned": (48, 64, _t), "offset": (48, 64, _off4), "w62": (48, 62, _t), "odd_n": (33, 47, _t)}
_ref_cache = {}


def _device(model, pr, T, cfg, valid, dev, put=_t):
    a = (put(pr["Xf"], dev), put(pr["Xk"], dev), _t(T, dev), put(pr["Qk"], dev), _t(valid, dev))
    if model == "ray":
        H, g, c = tracker.normal_equations(*a, cfg=cfg)
    else:
        H, g, c = tracker.normal_equations_calib(*a, pr["K"], pr["size"], cfg=cfg)
    H = H.cpu().numpy()
    assert np.array_equal(H, H.T)
    return H, g.cpu().numpy(), float(c)


def _reference(model, h, w, pn, name):
    """(validity clear of every margin, float64 (H, g, cost), bounds) - computed once, shared by the layouts of a shape."""
    key = (model, h, w, pn, name)
    if key not in _ref_cache:
        pr, T, cfg = TR.problem(model, h, w), TR.poses(model)[pn], TR.cfg_of(model, name)
        valid = TR.clear_margins(model, pr, T, cfg)
        s = TR.systems(model, pr, T, cfg, valid)
        twin = TR.twin_error(model, pr, T, cfg, valid)
        _ref_cache[key] = (valid, (s["H"], s["g"], s["cost"]), twin, TR.bounds(twin))
    return _ref_cache[key]


@pytest.mark.parametrize("layout", sorted(_LAYOUTS))
@pytest.mark.parametrize("model", ["ray", "calib"])
def test_row_isolated_normal_equations(dev, model, layout):
    h, w, put = _LAYOUTS[layout]
    pr = TR.problem(model, h, w)
    bad = []
    for pn, T in TR.poses(model).items():
        for name in TR.CONFIGS[model]:
            valid, ref, twin, tol = _reference(model, h, w, pn, name)
            got = _device(model, pr, T, TR.cfg_of(model, name), valid, dev, put)
            r = TR.rel_err(got, ref)
            print(f"rows {model} {layout} {pn} {name}: H {r[0]:.3e} g {r[1]:.3e} cost {r[2]:.3e}  (twin {twin[0]:.1e} {twin[1]:.1e} "
                  f"{twin[2]:.1e}; bounds {tol[0]:.1e} {tol[1]:.1e} {tol[2]:.1e})")
            if not all(np.isfinite(x) and x <= t for x, t in zip(r, tol)):
                bad.append((pn, name, r, tol))
    assert not bad, bad


@pytest.mark.parametrize("shape", TR.ONE_HOT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("model", ["ray", "calib"])
def test_one_hot_points(dev, model, shape):
    """Validity is ONE point: its H, g and cost against its own float64 contribution, relative to its own max|H|, max|g|
    and cost - a wrong pixel for lanes 1..3 of a group, a wrong row at a row boundary or a slipped xyz unpacking is the
    whole signal.  8x12: the group loop; 5x7: the one-point loop."""
    h, w = shape
    pr, T = TR.problem(model, h, w, one_hot=True), TR.one_hot_pose()
    bad, worst = [], {}
    for name in TR.ONE_HOT_CONFIGS[model]:
        tol = TR.bounds(TR.one_hot_twin_error(model, h, w, name))
        for n, ref in TR.one_hot_reference(model, h, w, name):
            got = _device(model, pr, T, TR.one_hot_cfg(model, name), TR.one_hot(h * w, n), dev)
            r = TR.rel_err(got, ref)
            worst[name] = np.maximum(worst.get(name, 0.0), r)
            if not all(np.isfinite(x) and x <= t for x, t in zip(r, tol)):
                bad.append((name, n, r, tol))
        print(f"one-hot {model} {h}x{w} {name}: worst H {worst[name][0]:.3e} g {worst[name][1]:.3e} cost {worst[name][2]:.3e}  "
              f"(bounds {tol[0]:.1e} {tol[1]:.1e} {tol[2]:.1e})")
    assert not bad, bad


@pytest.mark.parametrize("name", ["default", "depth_mixed"])
def test_a_point_rejected_by_one_gate_contributes_exact_zeros(dev, name):
    pr, cfg = TR.problem("calib", 48, 64), TR.cfg_of("calib", name)
    pts = TR.gate_points(name)
    assert len(pts) == 6                            # u low / high, v low / high, p.z <= eps < zk, zk <= eps < p.z
    bad = []
    for gate, (pn, n) in pts.items():
        H, g, c = _device("calib", pr, TR.poses("calib")[pn], cfg, TR.one_hot(48 * 64, n), dev)
        if H.any() or g.any() or c != 0.0:
            bad.append((gate, pn, n, np.abs(H).max(), np.abs(g).max(), c))
    print(f"gates {name}: {pts}")
    assert not bad, bad


@pytest.mark.parametrize("P", [4100, 4098])
@pytest.mark.parametrize("name", sorted(TR.BLOCKS))
def test_backend_calibrated_blocks_depth_row(dev, name, P):
    """gn_point<2> with the depth row carrying each block (pixel sigma 1e4), Huber on it engaged everywhere / nowhere, on
    the four-point loop (P = 4100) and the one-point loop (4098).  Counts exact; H and g per edge."""
    (Twc, Xs, Cs, ii, jj, idx, valid, Q), _, (ct, qt) = TR.chain_scene(P)
    _, dcal = TR.blocks_calib(P, name)
    bl = kernels.gn_rays_blocks(Twc, Xs, Cs, ii, jj, idx, valid, Q, 1.0, ct, qt, point_mode=2, calib=dcal)
    ref, twin = TR.blocks_oracle(P, name), TR.blocks_twin_error(P, name)
    iu = np.triu_indices(7)
    rh = [np.abs(bl[e, :28] - H[iu]).max() / np.abs(H).max() for e, (H, g, n) in enumerate(ref)]
    rg = [np.abs(bl[e, 28:35] - g).max() / np.abs(g).max() for e, (H, g, n) in enumerate(ref)]
    print(f"blocks {name} P={P}: max H ratio {max(rh):.3e}, max g ratio {max(rg):.3e}  (twin H {max(t[0] for t in twin):.1e} "
          f"g {max(t[1] for t in twin):.1e})")
    for e, (H, g, n) in enumerate(ref):
        assert n > 1000 and bl[e, 35] == n
        assert rh[e] <= max(TR.FLOOR_BLOCKS, TR.TWIN_FACTOR * twin[e][0]), (e, rh[e])
        assert rg[e] <= max(TR.FLOOR_BLOCKS, TR.TWIN_FACTOR * twin[e][1]), (e, rg[e])


@pytest.mark.parametrize("iters", [1, 2, 3])
def test_the_loop_follows_the_distance_row(dev, iters):
    """opt_pose_ray_dist_sim3 at the dist_mixed sigmas, between world poses whose relative pose has a translation: the
    distance row alone fixes the common rescaling of s and t, and only if the t it rescales is that of the relative pose."""
    pr = TR.loop_problem()
    cfg = dict(max_iters=iters, sigma_ray=TR.RAY["dist_mixed"]["sigma_ray"], sigma_dist=TR.RAY["dist_mixed"]["sigma_dist"])
    Tf, Trel, info = tracker.opt_pose_ray_dist_sim3(_t(pr["Xf"], dev), _t(pr["Xk"], dev), _t(pr["T_WCf"], dev), _t(pr["T_WCk"], dev),
                                                    _t(pr["Qk"], dev), _t(pr["valid"], dev), cfg, fixed_iters=True)
    To, Trel_o, io = TR.loop_oracle(iters)
    d = np.abs(Trel.cpu().numpy() - Trel_o)
    dw = np.abs(Tf.cpu().numpy() - To).max()
    print(f"loop {iters}: t {d[:3].max():.3e} q {d[3:7].max():.3e} s {d[7]:.3e} world {dw:.3e}")
    info = info.cpu().numpy()
    assert int(info[0]) == iters == io["iters"] and info[3] == 0.0
    assert d.max() <= TR.LOOP_POSE_TOL and dw <= TR.LOOP_WORLD_TOL
    assert abs(info[1] - io["costs"][-1]) <= 1e-3 * io["costs"][-1]
