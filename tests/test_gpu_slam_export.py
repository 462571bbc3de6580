"""GPU: the map and trajectory writers under the SLAM driver (reference slam.py:320-415).  TINY_CFG random weights on
128x256 frames, as tests/test_gpu_slam_loop.py builds them: geometry is meaningless, what is checked is that the files
hold what results() and the keyframes' own confidences say they should."""
import numpy as np
import pytest
import torch

from mast3r_slam import config, model as M, synthetic
from mast3r_slam.slam import SLAM

pytestmark = pytest.mark.gpu
H, W = 128, 256
PLY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])


@pytest.fixture(scope="module")
def slam(dev):
    net = M.Mast3rFull(weights=M.init_random_weights(M.TINY_CFG, seed=1), cfg=M.TINY_CFG, device=dev)
    config.set_config({})
    s = SLAM(net)
    s.run([(0.1 * k, torch.from_numpy(synthetic.textured_image(H, W, 40 + k))) for k in range(5)])
    return s


def read_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines()
    assert lines[1] == "format binary_little_endian 1.0"
    m = int(lines[2].split()[-1])
    body = np.frombuffer(raw, dtype=PLY_DTYPE, offset=end)
    assert body.shape == (m,) and len(raw) == end + 15 * m
    return np.stack([body["x"], body["y"], body["z"]], axis=1), np.stack([body["red"], body["green"], body["blue"]], axis=1)


def test_save_pointcloud_without_threshold_is_results_points(slam, tmp_path):
    k = len(slam.keyframes)
    ref = slam.results()["points"].cpu().numpy()
    assert ref.shape == (k * H * W, 3)
    finite = np.isfinite(ref).all(axis=1)
    n = slam.save_pointcloud(tmp_path / "all.ply", c_conf_threshold=None)
    pts, col = read_ply(tmp_path / "all.ply")
    assert n == pts.shape[0] == k * H * W - int((~finite).sum())
    scale = max(1.0, float(np.abs(ref[finite]).max()))
    err = float(np.abs(pts - ref[finite]).max())
    print(f"{k} keyframes, {n} vertices, {int((~finite).sum())} non-finite, max |diff| {err:.3g} at data magnitude {scale:.3g}")
    assert err <= 1e-5 * scale
    want = np.concatenate([kf.img.cpu().numpy().reshape(-1, 3) for kf in slam.keyframes._frames])   # uint8 [H,W,3] frames
    assert want.dtype == np.uint8
    assert np.array_equal(col, want[finite])
    p, c, i = slam.reconstruction(c_conf_threshold=None, return_index=True)
    assert np.array_equal(i.cpu().numpy(), np.nonzero(finite)[0]) and p.cpu().numpy().tobytes() == pts.tobytes()


def test_save_pointcloud_threshold_at_the_median_confidence(slam, tmp_path):
    conf = torch.cat([kf.get_average_conf().reshape(-1) for kf in slam.keyframes._frames]).cpu().numpy()
    finite = np.isfinite(slam.results()["points"].cpu().numpy()).all(axis=1)
    thr = float(np.median(conf[np.isfinite(conf)]))
    want = int(((conf > np.float32(thr)) & finite).sum())
    n = slam.save_pointcloud(tmp_path / "half.ply", c_conf_threshold=thr)
    pts, _ = read_ply(tmp_path / "half.ply")
    print(f"median confidence {thr:.6g}: {n} of {conf.size} vertices")
    assert n == pts.shape[0] == want and 0 < want < conf.size
    voxel = float(np.abs(pts).max()) / 1000.0                               # voxel coordinates stay far below 2^20
    thin = slam.save_pointcloud(tmp_path / "thin.ply", c_conf_threshold=thr, voxel_size=voxel, binary=True)
    assert 0 < thin <= n and read_ply(tmp_path / "thin.ply")[0].shape[0] == thin


def test_save_trajectory_writes_the_results_poses(slam, tmp_path):
    res = slam.results()
    poses = res["poses"].cpu().numpy()
    assert slam.save_trajectory(tmp_path / "traj.txt") == 5
    want = [" ".join(f"{float(v):.6f}" for v in [ts, *row[:7]]) for ts, row in zip(res["timestamps"], poses)]
    assert open(tmp_path / "traj.txt").read().splitlines() == want
    assert slam.save_trajectory(tmp_path / "kitti.txt", format="kitti") == 5
    rows = np.loadtxt(tmp_path / "kitti.txt").reshape(5, 3, 4)
    assert np.allclose(rows[:, :, 3], poses[:, :3], atol=1e-6)
    assert np.allclose(np.cbrt(np.linalg.det(rows[:, :, :3])), poses[:, 7], rtol=1e-3, atol=1e-4)
    k = len(slam.keyframes)
    assert slam.save_trajectory(tmp_path / "kf.txt", keyframes_only=True) == k
    kf = np.loadtxt(tmp_path / "kf.txt").reshape(k, 8)
    assert np.allclose(kf[:, 0], [res["timestamps"][i] for i in res["keyframe_indices"]], atol=1e-6)
    assert np.allclose(kf[:, 1:], slam.keyframes.get_poses().cpu().numpy()[:, :7], atol=1e-6)
    with pytest.raises(ValueError):
        slam.save_trajectory(tmp_path / "bad.txt", format="euroc")
