"""GPU: mesh smoothing on the meshes of the SLAM driver.  TINY_CFG random weights on 128x256 frames, every keyframe's
pointmap and pose overwritten in place with keyframes that see one surface (tests/consistency_twin.shared_scene), as
tests/test_gpu_slam_simplify.py does.  The driver's mesh methods keep their signatures (existing tests pin them), so the
smoothing is the module call on what they return.  What is checked: smooth_mesh takes the tuples SLAM.mesh and
SLAM.fused_mesh return, keeps their shapes, their faces and every finite vertex finite, and leaves the boundary where it
was with fix_boundary; vertex_normals, render_mesh(shading="headlight") and save_ply_mesh take its result as it is."""
import numpy as np
import pytest
import torch

import consistency_twin as CT
from mast3r_slam import config, export, fusion, mast3r_utils, model as M, normals, render, smooth, synthetic
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


def through(slam, mesh, tmp_path, name, **kw):
    """smooth_mesh on a driver mesh: shapes, faces, finiteness, the boundary, and the consumers downstream."""
    before = [t.clone() for t in mesh[:3]]
    out = smooth.smooth_mesh(mesh, **kw)
    assert len(out) == 3 and out[1] is mesh[1] and out[2] is mesh[2]
    assert out[0].shape == mesh[0].shape and out[0].dtype == torch.float32 and out[0].data_ptr() != mesh[0].data_ptr()
    assert all(torch.equal(a, b) for a, b in zip(mesh[:3], before))             # the input is as it was
    finite = torch.isfinite(mesh[0]).all(dim=1)
    assert bool(finite.any()) and bool(torch.isfinite(out[0][finite]).all())
    assert bool((out[0][finite] != mesh[0][finite]).any())                      # something moved
    top = smooth.mesh_topology(mesh[2], mesh[0].shape[0])
    assert top.edges > 0 and top.invalid_faces == 0
    if kw.get("fix_boundary"):
        assert bool(top.boundary.any())
        assert out[0][top.boundary].cpu().numpy().tobytes() == mesh[0][top.boundary].cpu().numpy().tobytes()
    assert torch.equal(smooth.smooth_mesh(*mesh[:3], **kw)[0], out[0])          # whole or unpacked, and twice
    n = normals.vertex_normals(out)
    assert n.shape == out[0].shape and bool((n != 0).any())
    kf = [k for k in slam.keyframes._frames if k.X_canon is not None][0]
    rgb, depth = render.render_mesh(out, kf.T_WC, CT.shared_pinhole(H, W), (H, W), shading="headlight")
    assert rgb.shape == (H, W, 3) and bool(torch.isfinite(depth).any())
    assert export.save_ply_mesh(tmp_path / name, *out) == (out[0].shape[0], out[2].shape[0])
    return out, top


def test_keyframe_mesh_through_the_smoother(slam, tmp_path):
    plain = slam.mesh()
    assert plain[2].shape[0] > 0
    out, top = through(slam, plain, tmp_path, "smooth.ply", fix_boundary=True)
    print(f"keyframe mesh: V {plain[0].shape[0]}, F {plain[2].shape[0]}, E {top.edges}, boundary edges {top.boundary_edges}, "
          f"non-manifold {top.nonmanifold_edges}, longest row {int(top.degree.max())}")
    assert top.boundary_edges > 0                                               # keyframe meshes are open sheets
    through(slam, slam.mesh(return_index=True), tmp_path, "smooth_indexed.ply", fix_boundary=True)   # the 4-tuple, whole
    again = slam.mesh()
    assert all(torch.equal(a, b) for a, b in zip(again, plain))                 # the producer is as it was


def test_fused_mesh_through_the_smoother(slam, tmp_path):
    lo, hi = fusion.map_bounds(slam.keyframes)
    kw = dict(voxel_size=float((hi - lo).max()) / 64.0, bounds=(lo, hi))
    fused = slam.fused_mesh(**kw)
    assert fused[2].shape[0] > 0
    out, top = through(slam, fused, tmp_path, "fused_smooth.ply")
    print(f"fused mesh: V {fused[0].shape[0]}, F {fused[2].shape[0]}, E {top.edges}, boundary edges {top.boundary_edges}, "
          f"non-manifold {top.nonmanifold_edges}, longest row {int(top.degree.max())}")
    closed = top.boundary_edges == 0                                            # the README's test for a closed fused mesh
    assert closed == (not bool(top.boundary.any()))
    if not closed:                                                              # holes: their rims stay
        through(slam, fused, tmp_path, "fused_fixed.ply", fix_boundary=True)
    again = slam.fused_mesh(**kw)
    assert all(torch.equal(a, b) for a, b in zip(again, fused))                 # the producer is as it was


def test_re_exports():
    for n in ("smooth_mesh", "mesh_topology", "MeshTopology"):
        assert n in mast3r_utils.__all__ and getattr(mast3r_utils, n) is getattr(smooth, n)
