"""GPU: SLAM.estimate_intrinsics and render_view(K="estimate") on the synthetic loop of tests/test_gpu_slam_render.py
(TINY_CFG random weights, 128x256 frames).  Random weights give meaningless geometry, so after the run every keyframe's
pointmap is overwritten in place with what a pinhole of focal 200 sees (tests/focal_twin.py): the plumbing is what is
checked, on a map whose camera is known."""
import numpy as np
import pytest
import torch

import focal_twin as FT
from mast3r_slam import config, intrinsics, model as M, render, synthetic
from mast3r_slam.slam import SLAM

pytestmark = pytest.mark.gpu
H, W, FOCAL = 128, 256, 200.0
SIZE = (96, 160)
KW = dict(c_conf_threshold=None, point_size=3, background=(10, 20, 30))


@pytest.fixture(scope="module")
def slam(dev):
    net = M.Mast3rFull(weights=M.init_random_weights(M.TINY_CFG, seed=1), cfg=M.TINY_CFG, device=dev)
    config.set_config({})
    s = SLAM(net)
    s.run([(0.1 * k, torch.from_numpy(synthetic.textured_image(H, W, 40 + k))) for k in range(5)])
    kfs = [kf for kf in s.keyframes._frames if kf.X_canon is not None]
    assert kfs and all(kf.X_canon.shape == (H * W, 3) for kf in kfs)
    for i, kf in enumerate(kfs):
        X, C = FT.pinhole_keyframe(H, W, FOCAL, seed=70 + i, nk=int(kf.N))
        kf.X_canon.copy_(torch.from_numpy(X))
        kf.C.copy_(torch.from_numpy(C).reshape(kf.C.shape))
    return s


def test_slam_estimate_is_the_module_function_on_its_keyframes(slam):
    est = slam.estimate_intrinsics()
    ref = intrinsics.estimate_intrinsics(slam.keyframes)
    assert isinstance(est, intrinsics.IntrinsicsEstimate) and est.size == (H, W)
    assert est.principal_point == ((W - 1) / 2.0, (H - 1) / 2.0)
    assert est.focal == ref.focal and est.K.tobytes() == ref.K.tobytes()
    for name in ("focal_per_keyframe", "focal_lsq", "count", "residual_px"):
        assert getattr(est, name).tobytes() == getattr(ref, name).tobytes()
    rows = intrinsics.estimate_focal(slam.keyframes).cpu().numpy()
    assert rows[:, 0].tobytes() == est.focal_per_keyframe.tobytes() and est.focal == float(np.median(rows[:, 0]))
    print(f"{len(rows)} keyframes, focal {est.focal:.3f} (truth {FOCAL}), per keyframe {rows[:, 0].tolist()}")
    assert abs(est.focal - FOCAL) / FOCAL < 0.005                              # the bound of tests/test_focal_host.py
    few = slam.estimate_intrinsics(iters=0, c_conf_threshold=None, min_pixels=1)   # keywords reach the module function
    assert few.focal == float(np.median(few.focal_lsq)) and (few.count == H * W).all()
    with pytest.raises(ValueError, match="no keyframe"):
        slam.estimate_intrinsics(min_pixels=H * W + 1)


def test_render_view_with_the_estimate(slam, tmp_path):
    est = slam.estimate_intrinsics()
    T = slam.keyframes._frames[0].T_WC                                         # the first keyframe's camera sees its own pointmap
    for size in (SIZE, None):
        K = render.scaled_intrinsics(est.K, est.size, size or (H, W))
        a = slam.render_view(T, K="estimate", size=size, **KW)
        b = slam.render_view(T, K=K, size=size, **KW)
        assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))
        assert (a[0].cpu().numpy() != np.array([10, 20, 30], dtype=np.uint8)).any()
    assert slam.render_view(T, K="estimate", size=SIZE, **KW)[0].cpu().numpy().tobytes() != \
        slam.render_view(T, size=SIZE, **KW)[0].cpu().numpy().tobytes()         # 60 degrees is another camera
    slam.save_view(tmp_path / "est.png", T, K="estimate", size=SIZE, **KW)
    from PIL import Image
    assert np.asarray(Image.open(tmp_path / "est.png")).tobytes() == \
        slam.render_view(T, K="estimate", size=SIZE, **KW)[0].cpu().numpy().tobytes()
    with pytest.raises(ValueError, match="estimate"):
        slam.render_view(K="guess")


def test_render_view_without_k_is_unchanged(slam):
    pose = slam.poses[-1]
    for size in (SIZE, (H, W)):
        a = slam.render_view(size=size, **KW)
        b = render.render_map(slam.keyframes, pose, None, size, **KW)
        assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))
