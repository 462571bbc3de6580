"""GPU: the fused mesh under the SLAM driver.  TINY_CFG random weights on 128x256 frames, as tests/test_gpu_slam_mesh.py
builds them.  Random weights give meaningless geometry, so every keyframe's pointmap and pose are overwritten in place
with keyframes that see one surface (tests/consistency_twin.shared_scene), as tests/test_gpu_slam_consistency.py does:
what is checked is that the file holds what SLAM.fused_mesh() returns, that the indices are in range and that the call
leaves the point-cloud export as it was."""
import numpy as np
import pytest
import torch

import consistency_twin as CT
from mast3r_slam import config, fusion, model as M, synthetic
from mast3r_slam.slam import SLAM

pytestmark = pytest.mark.gpu
H, W = 128, 256
PLY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


@pytest.fixture(scope="module")
def slam(dev):
    net = M.Mast3rFull(weights=M.init_random_weights(M.TINY_CFG, seed=1), cfg=M.TINY_CFG, device=dev)
    config.set_config({})
    s = SLAM(net)
    s.run([(0.1 * k, torch.from_numpy(synthetic.textured_image(H, W, 40 + k))) for k in range(5)])
    return s


def read_ply_mesh(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines()
    assert lines[1] == "format binary_little_endian 1.0" and lines[10] == "property list uchar int vertex_indices"
    v, f = int(lines[2].split()[-1]), int(lines[9].split()[-1])
    assert lines[2] == f"element vertex {v}" and lines[9] == f"element face {f}" and len(raw) == end + 15 * v + 13 * f
    body = np.frombuffer(raw, dtype=PLY_DTYPE, count=v, offset=end)
    tri = np.frombuffer(raw, dtype=FACE_DTYPE, count=f, offset=end + 15 * v)
    assert (tri["n"] == 3).all()
    return (np.stack([body["x"], body["y"], body["z"]], axis=1).reshape(v, 3),
            np.stack([body["red"], body["green"], body["blue"]], axis=1).reshape(v, 3), tri["v"].reshape(f, 3))


def test_save_fused_mesh_writes_what_fused_mesh_returns_and_leaves_the_cloud_alone(slam, tmp_path):
    kfs = [kf for kf in slam.keyframes._frames if kf.X_canon is not None]
    K = len(kfs)
    sc = CT.shared_scene(K, H, W, seed=31)
    for i, kf in enumerate(kfs):                                              # in place: the driver's own tensors
        kf.X_canon.copy_(torch.from_numpy(sc["X"][i]))
        avg = sc["C"][i] / np.float32(sc["Nk"][i])
        kf.C.copy_(torch.from_numpy(avg * np.float32(kf.N)).reshape(kf.C.shape))
        kf.T_WC.copy_(torch.from_numpy(sc["T"][i]).reshape(kf.T_WC.shape))
    slam.save_pointcloud(tmp_path / "before.ply")
    # the defaults: the box of the exported points, 256 voxels along its longest side, trunc of 4 voxels
    v, c, f = slam.fused_mesh()
    n = slam.save_fused_mesh(tmp_path / "fused.ply")
    print(f"{K} keyframes: {v.shape[0]} vertices, {f.shape[0]} faces")
    assert n == (v.shape[0], f.shape[0]) and f.shape[0] > 0
    assert v.dtype == torch.float32 and c.dtype == torch.uint8 and f.dtype == torch.int32 and v.is_cuda
    assert v.shape[1:] == (3,) and c.shape == v.shape and f.shape[1:] == (3,)
    pv, pc, pf = read_ply_mesh(tmp_path / "fused.ply")
    assert pv.tobytes() == v.cpu().numpy().tobytes() and np.array_equal(pc, c.cpu().numpy())
    assert np.array_equal(pf, f.cpu().numpy())
    assert int(f.min()) >= 0 and int(f.max()) < v.shape[0]                     # indices in range
    # the module functions give the same mesh: the grid the driver chose, the pinhole it chose
    lo, hi = fusion.map_bounds(slam.keyframes)
    vs = float((hi - lo).max()) / 256.0
    pin = "estimate" if slam.keyframes.get_intrinsics() is None else slam.keyframes.get_intrinsics()
    volume = fusion.fuse_tsdf(slam.keyframes, pin, vs)
    assert max(volume.dims) in range(256, 256 + 12)                            # padded by trunc + voxel_size, snapped to the grid
    assert all(torch.equal(a, b) for a, b in zip(fusion.extract_surface(volume), (v, c, f)))
    assert bool((v >= torch.tensor(volume.origin).to(v)).all())
    # a coarser volume over explicit bounds, an ASCII file, a filtered map
    kw = dict(voxel_size=8 * vs, bounds=(lo, hi), min_weight=2)
    v2, c2, f2 = slam.fused_mesh(**kw)
    assert slam.save_fused_mesh(tmp_path / "coarse.ply", binary=False, **kw) == (v2.shape[0], f2.shape[0])
    assert 0 < f2.shape[0] < f.shape[0] and int(f2.max()) < v2.shape[0]
    v3, _, f3 = slam.fused_mesh(consistency=True if K >= 3 else dict(min_views=min(1, K - 1)), **kw)
    assert f3.numel() == 0 or int(f3.max()) < v3.shape[0]
    slam.save_pointcloud(tmp_path / "after.ply")
    assert open(tmp_path / "before.ply", "rb").read() == open(tmp_path / "after.ply", "rb").read()
