"""GPU: the mesh writer under the SLAM driver.  TINY_CFG random weights on 128x256 frames, as tests/test_gpu_slam_export.py
builds them: geometry is meaningless, what is checked is that the file holds what SLAM.mesh() returns and that the mesh
call leaves the point-cloud export as it was."""
import numpy as np
import pytest
import torch

from mast3r_slam import config, model as M, synthetic
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


def test_save_mesh_writes_what_mesh_returns_and_leaves_the_cloud_alone(slam, tmp_path):
    # random weights give random geometry: no threshold and a generous edge ratio, so that faces exist at all
    kw = dict(c_conf_threshold=None, stride=2, edge_ratio=1.0)
    slam.save_pointcloud(tmp_path / "before.ply", c_conf_threshold=None)
    v, c, f, i = slam.mesh(return_index=True, **kw)
    n = slam.save_mesh(tmp_path / "mesh.ply", **kw)
    print(f"{len(slam.keyframes)} keyframes: {v.shape[0]} vertices, {f.shape[0]} faces")
    assert n == (v.shape[0], f.shape[0])
    pv, pc, pf = read_ply_mesh(tmp_path / "mesh.ply")
    assert pv.tobytes() == v.cpu().numpy().tobytes() and np.array_equal(pc, c.cpu().numpy())
    assert np.array_equal(pf, f.cpu().numpy())
    assert v.dtype == torch.float32 and c.dtype == torch.uint8 and f.dtype == torch.int32 and i.dtype == torch.int64
    if f.shape[0]:
        assert int(f.min()) >= 0 and int(f.max()) < v.shape[0]
        p, _, pi = slam.reconstruction(c_conf_threshold=None, return_index=True)
        rows = torch.searchsorted(pi, i)
        assert torch.equal(pi[rows], i) and torch.equal(p[rows], v)             # the exporter's points
    assert slam.save_mesh(tmp_path / "default.ply") == tuple(t.shape[0] for t in slam.mesh()[::2])
    read_ply_mesh(tmp_path / "default.ply")
    slam.save_pointcloud(tmp_path / "after.ply", c_conf_threshold=None)
    assert open(tmp_path / "before.ply", "rb").read() == open(tmp_path / "after.ply", "rb").read()
