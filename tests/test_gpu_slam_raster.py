"""GPU: the `surface` keyword of SLAM.render_view / save_view and ViewRecorder, on the synthetic loop of
tests/test_gpu_slam_render.py (TINY_CFG random weights, 128x256 frames: geometry is meaningless, what is checked is the
plumbing)."""
import numpy as np
import pytest
import torch
from PIL import Image

import consistency_twin as CT
from mast3r_slam import config, model as M, render, synthetic
from mast3r_slam.slam import SLAM

pytestmark = pytest.mark.gpu
H, W = 128, 256
SIZE = (96, 160)
BG = (10, 20, 30)


def make(dev):
    net = M.Mast3rFull(weights=M.init_random_weights(M.TINY_CFG, seed=1), cfg=M.TINY_CFG, device=dev)
    config.set_config({})
    return SLAM(net)


def frames():
    return [(0.1 * k, torch.from_numpy(synthetic.textured_image(H, W, 40 + k))) for k in range(5)]


def test_surfaces_under_the_slam_loop(dev, tmp_path):
    # during the loop the pointmaps are random: keep every point, and every triangle whatever its shape
    loose = dict(c_conf_threshold=None, edge_ratio=1e6)
    rec = render.ViewRecorder(tmp_path, every=2, camera="frame", size=SIZE, surface="mesh", mesh_kw=loose, background=BG)
    s = make(dev)
    s.run(frames(), rec)
    names = sorted(p.name for p in tmp_path.glob("view_*.png"))
    assert names == ["view_000000.png", "view_000002.png", "view_000004.png"] and rec.calls == 5
    assert all(np.asarray(Image.open(tmp_path / n)).shape == (*SIZE, 3) for n in names)

    # keyframes that see one surface, written in place (as tests/test_gpu_slam_fusion.py does), seen from the first one
    # at 3 x the keyframes' size: there are fewer points than pixels
    kfs = [kf for kf in s.keyframes._frames if kf.X_canon is not None]
    sc = CT.shared_scene(len(kfs), H, W, seed=31)
    for i, kf in enumerate(kfs):
        kf.X_canon.copy_(torch.from_numpy(sc["X"][i]))
        kf.C.copy_(torch.from_numpy(sc["C"][i] / np.float32(sc["Nk"][i]) * np.float32(kf.N)).reshape(kf.C.shape))
        kf.T_WC.copy_(torch.from_numpy(sc["T"][i]).reshape(kf.T_WC.shape))
    pose, size = kfs[0].T_WC, (3 * H, 3 * W)
    K = render.scaled_intrinsics(CT.shared_pinhole(H, W), (H, W), size)
    points = s.render_view(pose, K, size, c_conf_threshold=None, background=BG)
    again = s.render_view(pose, K, size, surface="points", c_conf_threshold=None, background=BG)
    assert len(points) == 2 and all(torch.equal(a, b) for a, b in zip(points, again))
    covered = {"points": int(torch.isfinite(points[1]).sum())}
    kws = {"mesh": dict(c_conf_threshold=None, edge_ratio=0.05), "fused": dict(c_conf_threshold=None)}
    for surface, kw in kws.items():
        rgb, depth, index = s.render_view(pose, K, size, surface=surface, mesh_kw=kw, background=BG, return_index=True)
        assert rgb.shape == (*size, 3) and depth.shape == size and index.shape == size and rgb.dtype == torch.uint8
        assert torch.equal(index >= 0, torch.isfinite(depth))
        assert (rgb[index < 0] == torch.tensor(BG, dtype=torch.uint8, device=dev)).all()
        covered[surface] = int((index >= 0).sum())
    print(f"covered pixels of {size[0] * size[1]}: {covered}")
    assert covered["mesh"] > covered["points"] > 0 and covered["fused"] > covered["points"]

    K = render.scaled_intrinsics(CT.shared_pinhole(H, W), (H, W), SIZE)
    s.save_view(tmp_path / "mesh.png", pose, K, SIZE, surface="mesh", mesh_kw=kws["mesh"], background=BG)
    want = s.render_view(pose, K, SIZE, surface="mesh", mesh_kw=kws["mesh"], background=BG)[0].cpu().numpy()
    assert np.asarray(Image.open(tmp_path / "mesh.png")).tobytes() == want.tobytes()
    assert len(s.render_view(surface="mesh", mesh_kw=loose)) == 2              # defaults: last pose, the keyframes' size
    with pytest.raises(ValueError, match="surface"):
        s.render_view(size=SIZE, surface="bogus")
