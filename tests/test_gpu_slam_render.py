"""GPU: a ViewRecorder as the callback of SLAM.run, on the synthetic loop of tests/test_gpu_slam_export.py (TINY_CFG random
weights, 128x256 frames: geometry is meaningless, what is checked is the plumbing)."""
import numpy as np
import pytest
import torch
from PIL import Image

from mast3r_slam import config, model as M, render, synthetic
from mast3r_slam.slam import SLAM

pytestmark = pytest.mark.gpu
H, W = 128, 256
SIZE = (96, 160)


KW = dict(c_conf_threshold=None, point_size=3, background=(10, 20, 30))


def make(dev):
    net = M.Mast3rFull(weights=M.init_random_weights(M.TINY_CFG, seed=1), cfg=M.TINY_CFG, device=dev)
    config.set_config({})
    return SLAM(net)


def frames():
    return [(0.1 * k, torch.from_numpy(synthetic.textured_image(H, W, 40 + k))) for k in range(5)]


def test_view_recorder_under_the_slam_loop(dev, tmp_path):
    rec = render.ViewRecorder(tmp_path, every=2, camera="follow", size=SIZE, follow_distance=0.5, follow_height=0.1, **KW)
    s, views = make(dev), []

    def callback(frame, keyframes):
        # the backend runs after the callback and may move keyframes: SLAM.render_view is taken here, on the map the
        # recorder has just drawn
        if rec(frame, keyframes) is not None:
            views.append(s.render_view(rec.last_pose, size=SIZE, **KW)[0].cpu().numpy())

    res = s.run(frames(), callback)
    names = sorted(p.name for p in tmp_path.glob("view_*.png"))
    assert names == ["view_000000.png", "view_000002.png", "view_000004.png"] and rec.calls == 5 and len(views) == 3
    imgs = [np.asarray(Image.open(tmp_path / n)) for n in names]
    assert all(a.shape == (*SIZE, 3) and a.dtype == np.uint8 for a in imgs)
    assert imgs[-1].tobytes() == views[-1].tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(imgs, views))
    drawn = (imgs[-1] != np.array([10, 20, 30], dtype=np.uint8)).any(axis=2).mean()
    print(f"last view: {100 * drawn:.1f} % of the pixels drawn")
    res2 = make(dev).run(frames())                                            # the recorder does not disturb the loop
    assert res["timestamps"] == res2["timestamps"] and res["keyframe_indices"] == res2["keyframe_indices"]
    assert res["poses"].cpu().numpy().tobytes() == res2["poses"].cpu().numpy().tobytes()
    assert res["points"].cpu().numpy().tobytes() == res2["points"].cpu().numpy().tobytes()
    rgb, depth = s.render_view()                                              # defaults: last pose, the keyframes' size
    assert rgb.shape == (H, W, 3) and depth.shape == (H, W)
    s.save_view(tmp_path / "final.png", size=SIZE, **KW)
    assert np.asarray(Image.open(tmp_path / "final.png")).shape == (*SIZE, 3)
