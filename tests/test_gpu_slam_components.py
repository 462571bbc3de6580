"""GPU: the mesh clean-up on the meshes of the SLAM driver.  TINY_CFG random weights on 128x256 frames, every keyframe's
pointmap and pose overwritten in place with keyframes that see one surface (tests/consistency_twin.shared_scene), as
tests/test_gpu_slam_fusion.py does.  The driver's mesh methods keep their signatures (existing tests pin them), so the
clean-up is the module call on what they return.  What is checked: filter_components takes the tuples SLAM.mesh and
SLAM.fused_mesh return, whole or unpacked, and equals the numpy twin on them; the README's one-liners write those
bytes; the producers and the point-cloud export are left as they were."""
import numpy as np
import pytest
import torch

import components_twin as CC
import consistency_twin as CT
from mast3r_slam import components, config, export, fusion, model as M, synthetic
from mast3r_slam.slam import SLAM

pytestmark = pytest.mark.gpu
H, W = 128, 256
PLY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def read_ply_mesh(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines()
    assert lines[1] == "format binary_little_endian 1.0" and lines[10] == "property list uchar int vertex_indices"
    v, f = int(lines[2].split()[-1]), int(lines[9].split()[-1])
    assert len(raw) == end + 15 * v + 13 * f
    body = np.frombuffer(raw, dtype=PLY_DTYPE, count=v, offset=end)
    tri = np.frombuffer(raw, dtype=FACE_DTYPE, count=f, offset=end + 15 * v)
    assert (tri["n"] == 3).all()
    return (np.stack([body["x"], body["y"], body["z"]], axis=1).reshape(v, 3),
            np.stack([body["red"], body["green"], body["blue"]], axis=1).reshape(v, 3), tri["v"].reshape(f, 3))


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


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


def check_against_twin(mesh, **kw):
    want = CC.filter_mesh(*(t.cpu().numpy() for t in mesh[:3]), **kw)
    got = components.filter_components(mesh, return_index=True, **kw)
    assert got[0].cpu().numpy().tobytes() == want[0].tobytes() and all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got[1:], want[1:]))
    assert same(got[:3], components.filter_components(*mesh[:3], **kw))         # whole or unpacked
    return got


def write_and_read_back(path, mesh):
    n = export.save_ply_mesh(path, *mesh)
    pv, pc, pf = read_ply_mesh(path)
    assert n == (mesh[0].shape[0], mesh[2].shape[0])
    assert pv.tobytes() == mesh[0].cpu().numpy().tobytes() and np.array_equal(pc, mesh[1].cpu().numpy())
    assert np.array_equal(pf, mesh[2].cpu().numpy())


def test_keyframe_mesh_through_the_filter(slam, tmp_path):
    slam.save_pointcloud(tmp_path / "before.ply")
    plain = slam.mesh()
    assert plain[2].shape[0] > 0
    labels, faces_of, info = components.mesh_components(plain[2], plain[0].shape[0])
    print(f"{plain[0].shape[0]} vertices, {plain[2].shape[0]} faces, {info}")
    assert info.components >= 1 and int(faces_of.max()) == info.largest and int(labels.min()) == 0
    kept = check_against_twin(plain, min_faces=5)
    largest = check_against_twin(plain, largest_only=True)
    assert largest[2].shape[0] == info.largest <= kept[2].shape[0] <= plain[2].shape[0]
    check_against_twin(plain, min_fraction=0.25, min_faces=3)
    # the source index of a kept vertex: the producer's index at the kept rows
    indexed = slam.mesh(return_index=True)
    assert same(indexed[:3], plain)
    got = components.filter_components(indexed, min_faces=5, return_index=True)  # the 4-tuple, whole: its index is not a mesh array
    assert same(got, kept) and indexed[3][got[3]].shape == (kept[0].shape[0],)
    # a stride and a consistency filter ahead of it
    K = len([kf for kf in slam.keyframes._frames if kf.X_canon is not None])
    coarse = slam.mesh(stride=2, consistency=True if K >= 3 else dict(min_views=min(1, K - 1)))
    if coarse[2].shape[0]:
        check_against_twin(coarse, largest_only=True)
    # the README's one-liner writes those bytes
    write_and_read_back(tmp_path / "clean.ply", components.filter_components(slam.mesh(), min_faces=5))
    assert same(slam.mesh(), plain)                                             # the producer is as it was
    slam.save_pointcloud(tmp_path / "after.ply")
    assert open(tmp_path / "before.ply", "rb").read() == open(tmp_path / "after.ply", "rb").read()


def test_fused_mesh_through_the_filter(slam, tmp_path):
    slam.save_pointcloud(tmp_path / "before.ply")
    lo, hi = fusion.map_bounds(slam.keyframes)
    kw = dict(voxel_size=float((hi - lo).max()) / 64.0, bounds=(lo, hi))
    fused = slam.fused_mesh(**kw)
    assert fused[2].shape[0] > 0
    clean = check_against_twin(fused, largest_only=True)[:3]
    info = components.mesh_components(fused[2], fused[0].shape[0])[2]
    again = components.mesh_components(clean[2], clean[0].shape[0])[2]
    print(f"fused: {fused[2].shape[0]} faces, {info}; kept {clean[2].shape[0]}")
    assert again == (1, info.largest, 0) and clean[2].shape[0] == info.largest
    write_and_read_back(tmp_path / "fused_clean.ply", components.filter_components(slam.fused_mesh(**kw), largest_only=True))
    assert same(slam.fused_mesh(**kw), fused)                                   # the producer is as it was
    slam.save_pointcloud(tmp_path / "after.ply")
    assert open(tmp_path / "before.ply", "rb").read() == open(tmp_path / "after.ply", "rb").read()
