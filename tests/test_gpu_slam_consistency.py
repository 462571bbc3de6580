"""GPU: the consistency option of the map writers under the SLAM driver.  TINY_CFG random weights on 128x256 frames, as
tests/test_gpu_slam_mesh.py builds them.  Random weights give meaningless geometry, so for the filtered calls every
keyframe's pointmap and pose are overwritten in place with keyframes that see one surface
(tests/consistency_twin.shared_scene): the plumbing is what is checked."""
import numpy as np
import pytest
import torch

import consistency_twin as CT
from mast3r_slam import config, consistency, export, model as M, synthetic
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
    m = int(lines[2].split()[-1])
    assert lines[2] == f"element vertex {m}"
    body = np.frombuffer(raw, dtype=PLY_DTYPE, count=m, offset=end)
    return m, np.stack([body["x"], body["y"], body["z"]], axis=1), len(raw) - end


def test_consistency_none_is_the_unfiltered_call(slam, tmp_path):
    kw = dict(c_conf_threshold=None)
    assert slam.save_pointcloud(tmp_path / "a.ply", **kw) == slam.save_pointcloud(tmp_path / "b.ply", consistency=None, **kw)
    assert open(tmp_path / "a.ply", "rb").read() == open(tmp_path / "b.ply", "rb").read()
    mkw = dict(c_conf_threshold=None, stride=2, edge_ratio=1.0)
    slam.save_mesh(tmp_path / "a_mesh.ply", **mkw)
    export.save_ply_mesh(tmp_path / "b_mesh.ply", *slam.mesh(consistency=None, **mkw))
    assert open(tmp_path / "a_mesh.ply", "rb").read() == open(tmp_path / "b_mesh.ply", "rb").read()
    a, b = slam.reconstruction(return_index=True), slam.reconstruction(return_index=True, consistency=None)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_filtered_cloud_is_a_subset_and_equals_the_module_functions(slam, tmp_path):
    kfs = [kf for kf in slam.keyframes._frames if kf.X_canon is not None]
    K = len(kfs)
    sc = CT.shared_scene(K, H, W, seed=31)
    for i, kf in enumerate(kfs):                                              # in place: the driver's own tensors
        kf.X_canon.copy_(torch.from_numpy(sc["X"][i]))
        avg = sc["C"][i] / np.float32(sc["Nk"][i])
        kf.C.copy_(torch.from_numpy(avg * np.float32(kf.N)).reshape(kf.C.shape))
        kf.T_WC.copy_(torch.from_numpy(sc["T"][i]).reshape(kf.T_WC.shape))
    rule = True if K >= 3 else dict(min_views=min(1, K - 1))                  # the defaults ask for two other views
    p0, _, i0 = slam.reconstruction(return_index=True)
    p1, c1, i1 = slam.reconstruction(return_index=True, consistency=rule)
    print(f"{K} keyframes: {i0.numel()} points, {i1.numel()} pass the filter")
    assert 0 < i1.numel() < i0.numel()
    sel = torch.isin(i0, i1)
    assert int(sel.sum()) == i1.numel() and torch.equal(p0[sel], p1)          # a subset, by index, with the same bytes
    pin = "estimate" if slam.keyframes.get_intrinsics() is None else slam.keyframes.get_intrinsics()
    kw = {} if rule is True else rule
    views = consistency.consistent_keyframes(slam.keyframes, pin, **kw)
    p2, c2, i2 = export.collect_map(views, return_index=True)
    assert torch.equal(i1, i2) and torch.equal(p1, p2) and torch.equal(c1, c2)
    n = slam.save_pointcloud(tmp_path / "f.ply", consistency=rule)
    m, pts, nbytes = read_ply(tmp_path / "f.ply")
    assert n == m == i1.numel() and nbytes == 15 * m and pts.tobytes() == p1.cpu().numpy().tobytes()
    # no threshold with a filter: every KEPT point, not every point
    views = consistency.consistent_keyframes(slam.keyframes, pin, c_conf_threshold=None, **kw)
    i3 = slam.reconstruction(c_conf_threshold=None, return_index=True, consistency=rule)[2]
    assert torch.equal(i3, export.collect_map(views, c_conf_threshold=float("-inf"), return_index=True)[2])
    assert i3.numel() < slam.reconstruction(c_conf_threshold=None, return_index=True)[2].numel()
    v, _, f, vi = slam.mesh(edge_ratio=0.2, return_index=True, consistency=rule)
    assert torch.isin(vi, i1).all() and (f.numel() == 0 or int(f.max()) < v.shape[0])
