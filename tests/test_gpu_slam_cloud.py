"""GPU: point-cloud normals and the radius filter on the cloud of the SLAM driver.  TINY_CFG random weights on 128x256
frames, every keyframe's pointmap and pose overwritten in place with keyframes that see one surface
(tests/consistency_twin.shared_scene), as tests/test_gpu_slam_smooth.py does.  The driver's methods keep their
signatures (existing tests pin them), so the new calls are applied to what SLAM.reconstruction returns - the README's
usage line.  What is checked: every normal is unit length or zero and faces the camera that saw its point, the filter
returns a subset in source order, save_ply_normals writes what it was given, and the producer is as it was."""
import numpy as np
import pytest
import torch

import consistency_twin as CT
from mast3r_slam import cloud, config, export, fusion, mast3r_utils, model as M, synthetic
from mast3r_slam.slam import SLAM

pytestmark = pytest.mark.gpu
H, W = 128, 256


@pytest.fixture(scope="module")
def slam(dev):
    net = M.Mast3rFull(weights=M.init_random_weights(M.TINY_CFG, seed=1), cfg=M.TINY_CFG, device=dev)
    config.set_config({})
    s = SLAM(net)
    s.run([(0.1 * k, torch.from_numpy(synthetic.textured_image(H, W, 40 + k))) for k in range(5)])
    kfs = [kf for kf in s.keyframes._frames if kf.X_canon is not None]
    sc = CT.shared_scene(len(kfs), H, W, seed=31)
    for i, kf in enumerate(kfs):                                              # in place: the driver's own tensors
        kf.X_canon.copy_(torch.from_numpy(sc["X"][i]))
        avg = sc["C"][i] / np.float32(sc["Nk"][i])
        kf.C.copy_(torch.from_numpy(avg * np.float32(kf.N)).reshape(kf.C.shape))
        kf.T_WC.copy_(torch.from_numpy(sc["T"][i]).reshape(kf.T_WC.shape))
    return s


def test_reconstruction_through_normals_filter_and_writer(slam, tmp_path):
    lo, hi = fusion.map_bounds(slam.keyframes)
    v = float((hi - lo).max()) / 128.0
    pts = slam.reconstruction(voxel_size=v, return_index=True)
    before = [t.clone() for t in pts]
    m = pts[0].shape[0]
    assert m > 1000
    toward = mast3r_utils.source_viewpoints(slam.keyframes, pts[2])
    kfs = [kf for kf in slam.keyframes._frames if kf.X_canon is not None]
    k = torch.div(pts[2], H * W, rounding_mode="floor")
    assert toward.shape == (m, 3) and toward.dtype == torch.float32
    assert torch.equal(toward, torch.cat([kf.T_WC.reshape(1, 8)[:, :3] for kf in kfs])[k])
    n, var = mast3r_utils.cloud_normals(pts, radius=3 * v, toward=toward, return_variation=True)
    assert n.shape == (m, 3) and n.dtype == torch.float32 and var.shape == (m,)
    length = n.double().norm(dim=1)
    zero = ~n.any(dim=1)
    assert bool(((length - 1.0).abs() <= 1e-6)[~zero].all()) and bool((var[zero] == 0).all())
    to = toward.double() - pts[0].double()
    facing = (n.double() * to).sum(dim=1) >= -1e-6 * to.norm(dim=1)
    assert bool(facing[~zero].all())
    nb = cloud.cloud_neighbors(pts[0], 3 * v)
    assert bool(zero[nb.count < 3].all()) and int(zero.sum()) < m // 2          # below min_points: no normal
    print(f"cloud: {m} points at voxel {v:.4f}, {int(zero.sum())} without a normal, mean neighbours "
          f"{float(nb.count.float().mean()):.1f}, max {int(nb.count.max())}, mean variation {float(var[~zero].mean()):.4f}")
    assert float(nb.count.float().mean()) > 5                                   # three voxel edges see the surface
    assert torch.equal(mast3r_utils.cloud_normals(pts, radius=3 * v, toward=toward), n)             # twice

    k_min = 8
    kept = mast3r_utils.remove_radius_outliers(pts, radius=3 * v, min_neighbors=k_min, return_rows=True)
    rows = kept[3]
    assert len(kept) == 4 and 0 < rows.shape[0] <= m and bool((rows[1:] > rows[:-1]).all())         # a subset in source order
    assert torch.equal(rows, torch.nonzero(nb.count - 1 >= k_min).reshape(-1))
    assert torch.equal(kept[0], pts[0][rows]) and torch.equal(kept[1], pts[1][rows]) and torch.equal(kept[2], pts[2][rows])
    pair = mast3r_utils.remove_radius_outliers(pts[0], pts[1], radius=3 * v, min_neighbors=k_min)
    assert len(pair) == 2 and torch.equal(pair[0], kept[0])

    path = tmp_path / "cloud_normals.ply"
    assert export.save_ply_normals(path, pts[0], pts[1], n) == m
    with open(path, "rb") as f:
        head = b""
        while not head.endswith(b"end_header\n"):
            head += f.readline()
        body = np.fromfile(f, dtype=export._PLY_NORMALS_DTYPE)
    assert f"element vertex {m}\n".encode() in head and b"property float nx" in head and b"element face" not in head
    assert body.shape == (m,)
    assert np.stack([body["x"], body["y"], body["z"]], axis=1).tobytes() == pts[0].cpu().numpy().tobytes()
    assert np.stack([body["nx"], body["ny"], body["nz"]], axis=1).tobytes() == n.cpu().numpy().tobytes()
    assert np.stack([body["red"], body["green"], body["blue"]], axis=1).tobytes() == pts[1].cpu().numpy().tobytes()

    assert all(torch.equal(a, b) for a, b in zip(pts, before))                  # the inputs are as they were
    again = slam.reconstruction(voxel_size=v, return_index=True)
    assert all(torch.equal(a, b) for a, b in zip(again, before))                # the producer is as it was


def test_re_exports():
    for n in ("cloud_neighbors", "cloud_normals", "source_viewpoints", "remove_radius_outliers", "CloudNeighbors"):
        assert n in mast3r_utils.__all__ and getattr(mast3r_utils, n) is getattr(cloud, n)
    assert mast3r_utils.save_ply_normals is export.save_ply_normals
