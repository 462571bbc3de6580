"""GPU: register_clouds on the cloud of the SLAM driver - the tiny synthetic run of tests/test_gpu_slam_cloud.py
(TINY_CFG random weights on 128x256 frames, every keyframe overwritten in place with keyframes that see one surface).
The driver's methods keep their signatures, so the new call is applied to what SLAM.reconstruction returns.

Every third point of the cloud is moved by a known Sim(3) and rounded to float32; registering it onto the whole cloud has
to give the inverse.  The surface of this run is ONE tilted plane with depth noise: nothing but the noise and the
outline holds a source in place along it, so the motion is kept inside the basin in which most nearest neighbours are the
points' own originals - 0.2 degrees about the centroid, 0.3 voxel edges, scale 1.004: at most 0.7 voxel edges at the rim,
where the nearest other point is 0.6 away in the median (tests/icp_twin.py's scenes carry the 5 degree case).  The bound
is the one recorded in tests/icp_twin.py, with the translation in units of the cloud's extent.  Point to plane
cannot see motion along a plane, so with the normals the test asks only that the plane residual comes down."""
import math

import numpy as np
import pytest
import torch

import icp_twin as IT
from mast3r_slam import fusion, mast3r_utils
from test_gpu_slam_cloud import slam  # noqa: F401  (the fixture: the same run)

pytestmark = pytest.mark.gpu


def known_motion(centre, v):
    g = np.random.default_rng(5)
    axis = g.normal(size=3)
    axis /= np.linalg.norm(axis)
    th = math.radians(0.2)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K
    t = g.normal(size=3)
    t *= 0.3 * v / np.linalg.norm(t)
    M = np.eye(4)
    M[:3, :3] = 1.004 * R
    M[:3, 3] = centre - 1.004 * R @ centre + t
    return M


def test_registration_brings_a_moved_subset_back(slam):  # noqa: F811
    lo, hi = fusion.map_bounds(slam.keyframes)
    v = float((hi - lo).max()) / 128.0
    pts = slam.reconstruction(voxel_size=v, return_index=True)
    before = [t.clone() for t in pts]
    ref = pts[0]
    m = ref.shape[0]
    assert m > 1000
    normals = mast3r_utils.cloud_normals(pts, radius=3 * v, toward=mast3r_utils.source_viewpoints(slam.keyframes, pts[2]))
    host = ref.cpu().numpy()
    M = known_motion(host.astype(np.float64).mean(axis=0), v)
    moved = mast3r_utils.Registration(M, 1.004, 1.0, 0.0, 0, True, "ok", None, None, 0).apply(ref[::3])
    assert moved.dtype == torch.float32 and moved.shape == ref[::3].shape
    want = (M[:3, :3] @ host[::3].astype(np.float64).T).T + M[:3, 3]
    assert np.array_equal(moved.cpu().numpy(), want.astype(np.float32))         # apply agrees with the matrix

    reg = mast3r_utils.register_clouds(moved, ref, radius=5 * v, method="point_to_point", target_normals=normals, with_scale=True,
                                       return_pairs=True)
    E = (reg.T @ M)[:3] - np.eye(4)[:3]
    extent = float(np.abs(host).max())
    err = max(float(np.abs(E[:, :3]).max()), float(np.abs(E[:, 3]).max()) / extent)
    print(f"cloud: {m} points at voxel {v:.4f}; point to point: {reg.iterations} iterations, status {reg.status}, fitness "
          f"{reg.fitness:.4f}, rmse {reg.inlier_rmse:.3e}, error {err:.3e}")
    assert reg.status == "ok" and reg.converged and reg.iterations < 30 and reg.out_of_range == 0
    assert err <= IT.MARGIN * max(IT.RECOVERY.values())
    assert reg.fitness == 1.0 and reg.inlier_rmse < 1e-6 * extent
    assert torch.equal(reg.pairs.long(), torch.arange(0, m, 3, device=ref.device))          # every row found its original
    back = reg.apply(moved)
    assert float((back.double() - ref[::3].double()).abs().max()) <= 4e-7 * extent          # float32 rounding, twice
    assert abs(reg.scale * 1.004 - 1.0) <= IT.MARGIN * max(IT.RECOVERY.values()) and reg.T.shape == (4, 4) and reg.T.dtype == np.float64
    again = mast3r_utils.register_clouds(moved, ref, radius=5 * v, method="point_to_point", with_scale=True)
    assert again.T.tobytes() == reg.T.tobytes() and again.history.tobytes() == reg.history.tobytes()

    # the documented recipe: normals given, point to plane.  On one plane only the residual along the normal is observable.
    plane = mast3r_utils.register_clouds(moved, ref, radius=5 * v, target_normals=normals, with_scale=True)
    print(f"point to plane: {plane.iterations} iterations, status {plane.status}, cost {plane.history[0, 1]:.3e} -> "
          f"{plane.history[-1, 1]:.3e}")
    assert plane.status == "ok" and plane.iterations >= 2 and plane.fitness > 0.9
    assert plane.history[-1, 1] < plane.history[0, 1] and 0 < plane.history[0, 0] <= moved.shape[0]
    assert plane.history.shape == (plane.iterations, 5) and abs(plane.scale - 1.0) < 0.1

    assert all(torch.equal(a, b) for a, b in zip(pts, before))                  # the inputs are as they were
    again = slam.reconstruction(voxel_size=v, return_index=True)
    assert all(torch.equal(a, b) for a, b in zip(again, before))                # the producer is as it was
