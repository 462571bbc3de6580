"""CPU: the focal estimate's float64 twin (tests/focal_twin.py) against the truth of its own scenes, the host module's
argument errors and median rule, and the exported symbols."""
import inspect

import numpy as np
import pytest
import torch

import focal_twin as FT
from mast3r_slam import _ffi, intrinsics, mast3r_utils
from mast3r_slam.frame import Frame


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("H,W,f", [(32, 48, 40.0), (48, 64, 70.0), (37, 53, 30.0), (64, 80, 55.0)])
def test_twin_recovers_the_focal_where_least_squares_does_not(H, W, f, seed):
    """The formula and the recipe mean something: with 3 % wild points the Weiszfeld focal after 10 steps is within
    0.5 % of the truth (measured worst case 0.13 %, x4 for another random stream) while the least-squares start is
    more than 20 % away (measured 26 ... 80 %)."""
    X, C = FT.pinhole_keyframe(H, W, f, seed, out_frac=0.03)
    fw, f0, count, resid = FT.focal_twin(X, C, 1, (H, W), thr=1.5, iters=10)
    print(f"{H}x{W} f={f} seed={seed}: weiszfeld {fw:.4f} ({100 * abs(fw - f) / f:.3f} %), lsq {f0:.4f} "
          f"({100 * abs(f0 - f) / f:.1f} %), {int(count)} pixels, residual {resid:.3f} px")
    assert abs(fw - f) / f < 0.005
    assert abs(f0 - f) / f > 0.20
    assert 0.5 * H * W < count < H * W and np.isfinite(resid)


def test_twin_on_hand_made_pixels():
    # 2 x 3 image, principal point (1, 0.5): pixels at u = -1, 0, 1 and v = -0.5, 0.5; exact pinhole of focal 2 at depth 4
    u, v = np.meshgrid([-1.0, 0.0, 1.0], [-0.5, 0.5])
    X = np.stack([u / 2 * 4, v / 2 * 4, np.full_like(u, 4.0)], axis=2).reshape(-1, 3)
    C = np.full(6, 2.0)
    assert FT.focal_twin(X, C, 1, (2, 3), iters=3).tolist() == [2.0, 2.0, 6.0, 0.0]
    assert FT.focal_twin(X, 2 * C, 2, (2, 3), iters=0).tolist() == [2.0, 2.0, 6.0, 0.0]
    assert FT.focal_twin(X, C, 1, (2, 3), thr=2.0)[2] == 0 and np.isnan(FT.focal_twin(X, C, 1, (2, 3), thr=2.0)[[0, 1, 3]]).all()
    assert FT.focal_twin(X, C, 1, (2, 3), thr=None, z_min=4.0)[2] == 0          # z > z_min is strict
    Xb = X.copy()
    Xb[0, 0], Xb[1, 1], Xb[2, 2], Xb[3, 2] = np.nan, np.inf, -np.inf, -1.0
    assert FT.focal_twin(Xb, C, 1, (2, 3))[2] == 2
    Cb = C.copy()
    Cb[0], Cb[1] = np.nan, 1.5
    assert FT.focal_twin(X, Cb, 1, (2, 3))[2] == 4 and FT.focal_twin(X, Cb, 1, (2, 3), thr=None)[2] == 6


def frame(i, n, img, count=1):
    f = Frame(frame_id=i, img=img, T_WC=torch.tensor([[0, 0, 0, 0, 0, 0, 1, 1.0]]))
    f.X_canon, f.C, f.N = torch.zeros(n, 3), torch.ones(n, 1), count
    return f


def test_argument_errors_come_before_anything_is_queued():
    kf = [frame(0, 20, torch.zeros(3, 4, 5))]
    for fn in (intrinsics.estimate_focal, intrinsics.estimate_intrinsics):
        for bad in (-1, 65, 2.5):
            with pytest.raises(ValueError, match="iters"):
                fn(kf, iters=bad)
        for bad in (-0.5, float("nan")):
            with pytest.raises(ValueError, match="z_min"):
                fn(kf, z_min=bad)
        for bad in ((4, 6), (5, 5), (0, 20), (20,)):
            with pytest.raises(ValueError, match="size"):
                fn(kf, size=bad)
        for bad in ((float("inf"), 1.0), (1.0, float("nan")), (1.0,)):
            with pytest.raises(ValueError, match="principal_point"):
                fn(kf, principal_point=bad)
        with pytest.raises(RuntimeError):                                     # valid, but on the CPU: there is no CPU path
            fn(kf, size=(4, 5))
    with pytest.raises(ValueError, match="no keyframe"):
        intrinsics.estimate_intrinsics([])
    assert intrinsics.estimate_focal([]).shape == (0, 4) and intrinsics.estimate_focal([]).dtype == torch.float64


def test_median_rule_on_hand_made_rows():
    nan = float("nan")
    rows = np.array([[50.0, 80.0, 5000, 0.4], [nan, nan, 0, nan], [70.0, 90.0, 1000, 0.5], [54.0, 70.0, 1024, 0.3],
                     [nan, 60.0, 4000, nan], [52.0, 75.0, 2000, 0.2], [58.0, 71.0, 9000, 0.6]])
    est = intrinsics.intrinsics_from_rows(rows, (48, 64), (31.5, 23.5))         # qualifying: 50, 54, 52, 58 -> even count
    assert est.focal == 53.0 == np.median([50.0, 54.0, 52.0, 58.0])
    assert est.K.dtype == np.float64 and np.array_equal(est.K, [[53.0, 0, 31.5], [0, 53.0, 23.5], [0, 0, 1]])
    assert est.principal_point == (31.5, 23.5) and est.size == (48, 64)
    assert np.array_equal(est.count, [5000, 0, 1000, 1024, 4000, 2000, 9000]) and est.count.dtype == np.int64
    assert np.array_equal(est.focal_per_keyframe, rows[:, 0], equal_nan=True)
    assert np.array_equal(est.focal_lsq, rows[:, 1], equal_nan=True) and np.array_equal(est.residual_px, rows[:, 3], equal_nan=True)
    assert intrinsics.intrinsics_from_rows(rows, (48, 64), (31.5, 23.5), min_pixels=1).focal == 54.0   # 70 joins: odd count
    with pytest.raises(ValueError, match=r"\[5000, 0, 1000, 1024, 4000, 2000, 9000\]"):
        intrinsics.intrinsics_from_rows(rows, (48, 64), (31.5, 23.5), min_pixels=10000)
    with pytest.raises(ValueError, match="no keyframe"):
        intrinsics.intrinsics_from_rows(np.zeros((0, 4)), (48, 64), (31.5, 23.5))


def test_symbols_are_declared_exported_and_validate():
    names = _ffi.declared_symbols()
    for n in ("m3_focal_ws_bytes", "m3_focal_launches", "m3_focal_estimate"):
        assert n in names
    for n in intrinsics.__all__:
        assert n in mast3r_utils.__all__ and getattr(mast3r_utils, n) is getattr(intrinsics, n)
    L = _ffi.lib()
    assert L.m3_abi_version() == 4000                                         # symbols were added, nothing changed
    assert L.m3_focal_ws_bytes(1, 4096) > 0 and L.m3_focal_ws_bytes(128, 512 * 512) > 0
    assert L.m3_focal_ws_bytes(2, 512 * 512) == 2 * L.m3_focal_ws_bytes(1, 512 * 512)
    assert L.m3_focal_ws_bytes(1, 2 ** 31 - 1) > 0 and L.m3_focal_ws_bytes(2 ** 15, 2 ** 16 - 1) > 0
    assert L.m3_focal_ws_bytes(2 ** 15, 2 ** 16) == 0 and L.m3_focal_ws_bytes(2, 2 ** 30) == 0    # K * N >= 2^31
    assert L.m3_focal_ws_bytes(0, 4096) == 0 and L.m3_focal_ws_bytes(1, 0) == 0
    assert len(L.m3_focal_launches.argtypes) == 1                            # a function of iters only
    counts = [L.m3_focal_launches(i) for i in range(65)]
    assert all(b >= a for a, b in zip(counts, counts[1:])) and counts[0] >= 1
    assert L.m3_focal_launches(-1) == 0 and L.m3_focal_launches(65) == 0      # out of range
    ok = [None, None, None, 1, 20, 4, 5, 1, 1.5, 2.0, 1.5, 0.0, 10, None, 0, None, None]
    assert L.m3_focal_estimate(*ok) == -1                                     # NULL pointers: refused before any launch
    k0 = list(ok)
    k0[3] = 0
    assert L.m3_focal_estimate(*k0) == 0                                      # K = 0 queues nothing
    for pos, bad in ((5, 5), (12, -1), (12, 65), (11, -1.0), (11, float("nan")), (9, float("inf")), (10, float("nan"))):
        a = list(k0)
        a[pos] = bad
        assert L.m3_focal_estimate(*a) == -1, (pos, bad)
    assert "min_pixels" in inspect.signature(intrinsics.estimate_intrinsics).parameters
