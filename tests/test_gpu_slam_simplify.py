"""GPU: mesh simplification on the meshes of the SLAM driver.  TINY_CFG random weights on 128x256 frames, every keyframe's
pointmap and pose overwritten in place with keyframes that see one surface (tests/consistency_twin.shared_scene), as
tests/test_gpu_slam_components.py does.  The driver's mesh methods keep their signatures (existing tests pin them), so
the simplification is the module call on what they return.  What is checked: simplify_mesh takes the tuples SLAM.mesh
and SLAM.fused_mesh return, whole or unpacked, equals the numpy twin on them and shrinks both counts at a voxel a few
times the mesh's own spacing; filter_components, vertex_normals, render_mesh and save_ply_mesh take its result as it is;
the producers and the point-cloud export are left as they were."""
import numpy as np
import pytest
import torch

import consistency_twin as CT
import simplify_twin as ST
from mast3r_slam import components, config, export, fusion, model as M, normals, render, simplify, synthetic
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


def check_against_twin(mesh, voxel):
    want = ST.simplify(*(t.cpu().numpy() for t in mesh[:3]), voxel)
    got = simplify.simplify_mesh(mesh, voxel_size=voxel, return_index=True)
    for g, w in zip(got, want[:5]):
        assert g.cpu().numpy().tobytes() == w.tobytes() and tuple(g.shape) == w.shape
    assert same(got[:3], simplify.simplify_mesh(*mesh[:3], voxel_size=voxel))   # whole or unpacked
    return got[:3]


def edge_length(mesh):
    """The median length of the first edge of every face: the mesh's own spacing."""
    v, f = mesh[0], mesh[2].long()
    return float((v[f[:, 1]] - v[f[:, 0]]).norm(dim=1).median())


def downstream(slam, small, tmp_path, name):
    """filter_components, vertex_normals, render_mesh and save_ply_mesh take the simplified mesh as it is."""
    clean = components.filter_components(small, largest_only=True)
    assert 0 < clean[2].shape[0] <= small[2].shape[0] and clean[0].shape[0] <= small[0].shape[0]
    n = normals.vertex_normals(small)
    assert n.shape == small[0].shape and bool((n != 0).any())
    kf = [k for k in slam.keyframes._frames if k.X_canon is not None][0]
    rgb, depth = render.render_mesh(small, kf.T_WC, CT.shared_pinhole(H, W), (H, W))
    assert rgb.shape == (H, W, 3) and bool(torch.isfinite(depth).any())
    assert export.save_ply_mesh(tmp_path / name, *small) == (small[0].shape[0], small[2].shape[0])
    pv, pc, pf = read_ply_mesh(tmp_path / name)
    assert pv.tobytes() == small[0].cpu().numpy().tobytes() and np.array_equal(pc, small[1].cpu().numpy())
    assert np.array_equal(pf, small[2].cpu().numpy())


def test_keyframe_mesh_through_the_simplifier(slam, tmp_path):
    slam.save_pointcloud(tmp_path / "before.ply")
    plain = slam.mesh()
    assert plain[2].shape[0] > 0
    voxel = 3.0 * edge_length(plain)
    small = check_against_twin(plain, voxel)
    print(f"keyframe mesh at voxel {voxel:.4g}: V {plain[0].shape[0]} -> {small[0].shape[0]}, F {plain[2].shape[0]} -> {small[2].shape[0]}")
    assert 0 < small[0].shape[0] < plain[0].shape[0] and 0 < small[2].shape[0] < plain[2].shape[0]
    indexed = slam.mesh(return_index=True)                                      # the 4-tuple, whole: its index is not a mesh array
    assert same(simplify.simplify_mesh(indexed, voxel_size=voxel), small)
    downstream(slam, small, tmp_path, "small.ply")
    assert same(slam.mesh(), plain)                                             # the producer is as it was
    slam.save_pointcloud(tmp_path / "after.ply")
    assert open(tmp_path / "before.ply", "rb").read() == open(tmp_path / "after.ply", "rb").read()


def test_fused_mesh_through_the_simplifier(slam, tmp_path):
    slam.save_pointcloud(tmp_path / "before.ply")
    lo, hi = fusion.map_bounds(slam.keyframes)
    grid = float((hi - lo).max()) / 64.0
    kw = dict(voxel_size=grid, bounds=(lo, hi))
    fused = slam.fused_mesh(**kw)
    assert fused[2].shape[0] > 0
    small = check_against_twin(fused, 3.0 * grid)
    print(f"fused mesh at voxel {3.0 * grid:.4g}: V {fused[0].shape[0]} -> {small[0].shape[0]}, F {fused[2].shape[0]} -> {small[2].shape[0]}")
    assert 0 < small[0].shape[0] < fused[0].shape[0] and 0 < small[2].shape[0] < fused[2].shape[0]
    downstream(slam, small, tmp_path, "fused_small.ply")
    # the README's one-liner: simplify, then keep the largest component
    clean = components.filter_components(simplify.simplify_mesh(slam.fused_mesh(**kw), voxel_size=3.0 * grid), largest_only=True)
    assert components.mesh_components(clean[2], clean[0].shape[0])[2].components == 1
    assert same(slam.fused_mesh(**kw), fused)                                   # the producer is as it was
    slam.save_pointcloud(tmp_path / "after.ply")
    assert open(tmp_path / "before.ply", "rb").read() == open(tmp_path / "after.ply", "rb").read()
