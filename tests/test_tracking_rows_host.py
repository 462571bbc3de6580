"""CPU only: the conditions under which tests/test_gpu_tracking_rows.py means something, asserted from the float64 oracle
alone (tests/tracking_rows.py), and the finding behind it: at the default sigmas the light residual row of both
tracking models sits below the 2e-5 tolerance of the aggregate tests, so nothing compared there sees its arithmetic."""
import numpy as np
import pytest

import tracking_rows as TR


def _cases(model):
    return [(h, w, pn, name) for (h, w) in TR.SHAPES for pn in TR.poses(model) for name in TR.CONFIGS[model]]


def _cleared(model, h, w, pn, name):
    pr, T, cfg = TR.problem(model, h, w), TR.poses(model)[pn], TR.cfg_of(model, name)
    valid = TR.clear_margins(model, pr, T, cfg)                          # raises above the 1 % cap
    s = TR.systems(model, pr, T, cfg, valid)
    return pr, T, cfg, valid, s, (valid & s["gated"] if model == "calib" else valid)


@pytest.mark.parametrize("model", ["ray", "calib"])
def test_the_light_row_is_below_the_aggregate_tolerance_at_the_default_sigmas(model):
    """The finding, as a regression guard: were the share above 2e-5 the aggregate tests would feel the row."""
    for h, w in TR.SHAPES:
        for pn, T in TR.poses(model).items():
            pr, cfg = TR.problem(model, h, w), TR.cfg_of(model, "default")
            s = TR.systems(model, pr, T, cfg)
            Hl, gl, cl = TR.rows_only(model, s, TR.LOW_ROW[model])
            share = (np.abs(Hl).max() / np.abs(s["H"]).max(), np.abs(gl).max() / np.abs(s["g"]).max(), cl / s["cost"])
            print(f"{model} {h}x{w} {pn} default: {TR.LOW_ROW[model]} row is {share[0]:.2e} of max|H|, {share[1]:.2e} of max|g|, "
                  f"{share[2]:.2e} of the cost; Huber on it: {TR.regime_shares(model, s, s['wr'].any(axis=1))[TR.LOW_ROW[model]]:.3f}")
            assert 0 < share[0] < TR.FLOOR_TRACK and share[1] < TR.FLOOR_TRACK and share[2] < TR.FLOOR_TRACK
            assert s["wr"][:, list(TR.ROWS[model][TR.LOW_ROW[model]])].max() < TR.HUBER        # its Huber branch never engages


@pytest.mark.parametrize("model", ["ray", "calib"])
def test_every_configuration_isolates_its_row_in_its_regime(model):
    for h, w, pn, name in _cases(model):
        pr, T, cfg, valid, s, contrib = _cleared(model, h, w, pn, name)
        spec = TR.CONFIGS[model][name]
        removed = int(pr["valid"].sum() - valid.sum())
        assert removed <= 0.01 * contrib.sum()                            # the 1 % cap (clear_margins raises above it)
        assert not TR.near_decision(model, pr, s, cfg)[valid].any()       # what is left is clear of every branch and gate
        assert contrib.sum() >= 0.5 * pr["valid"].sum() and contrib.sum() > 400
        reg = TR.regime_shares(model, s, contrib)
        twin = TR.twin_error(model, pr, T, cfg, valid)
        print(f"{model} {h}x{w} {pn} {name}: {int(contrib.sum())} points ({removed} on a margin), above k {reg}, "
              f"float32 twin H {twin[0]:.2e} g {twin[1]:.2e} cost {twin[2]:.2e}")
        if spec["regime"] is not None:
            cls, lo, hi, other = spec["regime"]
            assert lo <= reg[cls] <= hi, (h, w, pn, name, reg)
            assert all(reg[c] <= other for c in reg if c != cls), (h, w, pn, name, reg)
        if spec["target"] is not None:
            Ht, gt, ct = TR.rows_only(model, s, spec["target"])
            assert np.abs(Ht).max() >= 0.99 * np.abs(s["H"]).max() and np.abs(gt).max() >= 0.99 * np.abs(s["g"]).max()
            assert ct >= 0.99 * s["cost"]
        assert all(np.isfinite(t) and t < 1e-3 for t in twin)             # the twin is a usable yardstick


def test_every_gate_of_the_calibrated_model_fires_alone():
    """Over the poses of a shape: each of the six gates rejects at least 8 points that are valid and pass the other five
    (so both mixed cases of the two depth gates occur)."""
    for h, w in TR.SHAPES:
        alone = dict.fromkeys(("u_lo", "u_hi", "v_lo", "v_hi", "pz", "zk"), 0)
        for pn, T in TR.poses("calib").items():
            pr, cfg = TR.problem("calib", h, w), TR.cfg_of("calib", "default")
            s = TR.systems("calib", pr, T, cfg)
            g = TR.gate_passes(pr, s, cfg)
            assert np.array_equal(np.all(list(g.values()), axis=0), s["gated"])          # the six gates ARE the oracle's mask
            for k in g:
                alone[k] += int((pr["valid"] & ~g[k] & np.all([g[j] for j in g if j != k], axis=0)).sum())
        print(f"calib {h}x{w}: rejected by exactly one gate {alone}")
        assert all(n >= 8 for n in alone.values()), alone                # pz alone: p.z <= eps < zk; zk alone: zk <= eps < p.z


def test_gate_points_for_the_exact_zero_check():
    for name in ("default", "depth_mixed"):
        pts = TR.gate_points(name)
        assert sorted(pts) == ["pz", "u_hi", "u_lo", "v_hi", "v_lo", "zk"]
        for gate, (pn, n) in pts.items():
            pr, T, cfg = TR.problem("calib", 48, 64), TR.poses("calib")[pn], TR.cfg_of("calib", name)
            s = TR.systems("calib", pr, T, cfg)
            g = TR.gate_passes(pr, s, cfg)
            assert pr["valid"][n] and [k for k in g if not g[k][n]] == [gate]
            assert not TR.near_decision("calib", pr, s, cfg)[n]
            H, gg, c = TR.point_only(TR.systems("calib", pr, T, cfg, TR.one_hot(48 * 64, n)), n)
            assert not H.any() and not gg.any() and c == 0.0


@pytest.mark.parametrize("model", ["ray", "calib"])
def test_one_hot_points_pass_their_gates_clear_of_every_margin(model):
    T = TR.one_hot_pose()
    for h, w in TR.ONE_HOT_SHAPES:
        pos = TR.one_hot_positions(h, w)
        assert len(set(pos)) == 11 and pos[:4] == [0, 1, 2, 3] and pos[4] // w == 0 and pos[5] // w == 1 and pos[5] % w == 0
        assert pos[6:10] == list(range(h * w - 4, h * w)) and 0 < pos[10] // w < h - 1 and 0 < pos[10] % w < w - 1
        pr = TR.problem(model, h, w, one_hot=True)
        for name in TR.ONE_HOT_CONFIGS[model]:
            cfg = TR.cfg_of(model, name, **(TR.ONE_HOT_GATES if model == "calib" else {}))
            s = TR.systems(model, pr, T, cfg, np.ones(h * w, dtype=bool))
            assert not TR.near_decision(model, pr, s, cfg)[pos].any()
            if model == "calib":
                assert s["gated"][pos].all()
            spec, wr = TR.CONFIGS[model][name], s["wr"][pos]
            if spec["regime"] is not None:                                # every single point is in the configuration's regime
                rows = list(TR.ROWS[model][spec["regime"][0]])
                assert (wr[:, rows] >= TR.HUBER).all() if spec["regime"][1] > 0 else (wr < TR.HUBER).all()
            tw = TR.one_hot_twin_error(model, h, w, name)
            print(f"{model} one-hot {h}x{w} {name}: float32 twin (max over the points) H {tw[0]:.2e} g {tw[1]:.2e} cost {tw[2]:.2e}")
            assert all(np.isfinite(t) and t < 1e-3 for t in tw)


def test_backend_calibrated_block_configurations():
    for P in (4100, 4098):
        for name, spec in TR.BLOCKS.items():
            full, depth, og_ = TR.blocks_systems(P, name), TR.blocks_systems(P, name, rows=(0, 0, 1)), TR.blocks_oracle(P, name)
            tw = TR.blocks_twin_error(P, name)
            print(f"blocks P={P} {name}: counts {min(b[2] for b in full)}-{max(b[2] for b in full)}, float32 twin "
                  f"H {max(t[0] for t in tw):.2e} g {max(t[1] for t in tw):.2e}")
            assert len(full) == 12
            for (H, g, n, wr), (Hd, gd, _, _), (Ho, go, no) in zip(full, depth, og_):
                assert n == no and n > 1000
                # the restatement that carries the float32 twin is the oracle, to rounding
                assert np.abs(H - Ho).max() <= 1e-12 * np.abs(Ho).max() and np.abs(g - go).max() <= 1e-12 * np.abs(go).max()
                assert np.abs(Hd).max() >= 0.99 * np.abs(H).max() and np.abs(gd).max() >= 0.99 * np.abs(g).max()
                above = float((wr[:, 2] >= TR.HUBER).mean())
                assert spec["regime"][0] <= above <= spec["regime"][1] and not (wr[:, :2] >= TR.HUBER).any()
                assert np.abs(np.abs(wr[:, 2]) - TR.HUBER).min() > 1e-3 * TR.HUBER       # no point on the branch margin
            assert all(np.isfinite(t[0]) and np.isfinite(t[1]) for t in tw)


def test_the_loop_problem_needs_the_distance_row():
    """The relative pose the loop starts from has a translation, the loop has work to do in t and s, and the float32 twin
    of the loop is printed for the record (it holds t and s, not q: see TR.loop_twin_error)."""
    pr = TR.loop_problem()
    from oracle import sim3 as S
    T0 = S.sim3_mul_mlx(S.sim3_inv_mlx(pr["T_WCk"].astype(np.float64)), pr["T_WCf"].astype(np.float64))
    assert np.abs(T0[:3]).max() > 5e-3
    for it in (1, 2, 3):
        tw = TR.loop_twin_error(it)
        print(f"loop {it} iterations: float32 twin error t {tw[0]:.2e} q {tw[1]:.2e} s {tw[2]:.2e} world pose {tw[3]:.2e}")
        assert tw[0] < 1e-3 and tw[2] < 1e-3
    moved = np.abs(TR.loop_oracle(3)[1] - T0)
    assert moved[:3].max() > 0.02 and moved[7] > 0.01                     # the loop has work to do in t and s
    # the dist_mixed conditions hold on this problem at its starting pose too: the distance row carries the system
    cfg = TR.cfg_of("ray", "dist_mixed")
    s = TR.systems("ray", pr, T0, cfg)
    Hd, gd, cd = TR.rows_only("ray", s, "dist")
    assert np.abs(Hd).max() >= 0.99 * np.abs(s["H"]).max() and np.abs(gd).max() >= 0.99 * np.abs(s["g"]).max() and cd >= 0.99 * s["cost"]
