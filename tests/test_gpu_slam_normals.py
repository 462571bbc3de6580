"""GPU: vertex normals and lit views on the meshes of the SLAM driver.  TINY_CFG random weights on 128x256 frames, every
keyframe's pointmap and pose overwritten in place with keyframes that see one surface (tests/consistency_twin.shared_scene),
as tests/test_gpu_slam_components.py does.  What is checked: vertex_normals takes the tuples SLAM.mesh and SLAM.fused_mesh
return and gives unit or zero rows equal to the twin; the normals of one keyframe's mesh face its camera; render_view
draws lit views through its keywords; the README's one-liner writes a PLY whose normals read back equal."""
import numpy as np
import pytest
import torch

import consistency_twin as CT
import normals_twin as NT
from mast3r_slam import config, export, fusion, model as M, normals, synthetic
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


def unit_or_zero(n):
    length = np.linalg.norm(n.astype(np.float64), axis=1)
    zero = ~n.any(axis=1)
    assert np.isfinite(n).all() and (np.abs(length[~zero] - 1) < 2e-7).all()
    return zero


def check(mesh):
    got = normals.vertex_normals(mesh)
    assert got.shape == mesh[0].shape and got.dtype == torch.float32
    assert torch.equal(got, normals.vertex_normals(*mesh[:3]))                  # whole or unpacked
    n = got.cpu().numpy()
    assert n.tobytes() == NT.vertex_normals(mesh[0].cpu().numpy(), mesh[2].cpu().numpy()).tobytes()
    return n, unit_or_zero(n)


def test_normals_of_the_driver_meshes(slam):
    mesh = slam.mesh()
    assert mesh[2].shape[0] > 0
    n, zero = check(mesh)
    print(f"keyframe mesh: {len(n)} vertices, {int(zero.sum())} zero normals")
    assert not zero.all()
    lo, hi = fusion.map_bounds(slam.keyframes)
    fused = slam.fused_mesh(voxel_size=float((hi - lo).max()) / 64.0, bounds=(lo, hi))
    assert fused[2].shape[0] > 0
    n, zero = check(fused)
    print(f"fused mesh: {len(n)} vertices, {int(zero.sum())} zero normals")
    assert not zero.all()


def test_normals_of_one_keyframe_face_its_camera(slam):
    kf = [k for k in slam.keyframes._frames if k.X_canon is not None][0]
    mesh = export.collect_mesh([kf])
    assert mesh[2].shape[0] > 0
    n, zero = check(mesh)
    eye = kf.T_WC.reshape(-1)[:3].cpu().numpy().astype(np.float64)
    towards = (n.astype(np.float64) * (eye[None] - mesh[0].cpu().numpy().astype(np.float64))).sum(axis=1)
    assert (towards[~zero] > 0).all() and (~zero).sum() > 0


def test_lit_views_through_the_driver(slam, tmp_path):
    plain = slam.render_view(surface="mesh")
    lit = slam.render_view(surface="mesh", shading="headlight")
    assert lit[0].shape == (H, W, 3) and lit[0].dtype == torch.uint8 and lit[1].shape == (H, W)
    assert torch.equal(lit[1], plain[1]) and not torch.equal(lit[0], plain[0]) and torch.isfinite(plain[1]).any()
    as_colours = slam.render_view(surface="mesh", shading="normals")
    assert torch.equal(as_colours[1], plain[1]) and not torch.equal(as_colours[0], lit[0])
    clay = slam.render_view(surface="mesh", shading="headlight", shade_kw=dict(colors=None), size=(64, 128))
    assert clay[0].shape == (64, 128, 3)
    slam.save_view(tmp_path / "lit.png", surface="mesh", shading="headlight")
    assert (tmp_path / "lit.png").stat().st_size > 0
    with pytest.raises(ValueError, match="shading"):
        slam.render_view(surface="points", shading="headlight")
    assert all(torch.equal(a, b) for a, b in zip(slam.render_view(surface="mesh"), plain))


def test_ply_with_normals_of_the_driver_mesh(slam, tmp_path):
    mesh = slam.mesh()
    n = normals.vertex_normals(mesh)
    assert export.save_ply_mesh_normals(tmp_path / "mesh.ply", *mesh, n) == (mesh[0].shape[0], mesh[2].shape[0])
    pv, pn, pc, pf = NT.read_ply_mesh_normals(tmp_path / "mesh.ply")
    assert pv.tobytes() == mesh[0].cpu().numpy().tobytes() and pn.tobytes() == n.cpu().numpy().tobytes()
    assert np.array_equal(pc, mesh[1].cpu().numpy()) and np.array_equal(pf, mesh[2].cpu().numpy())
