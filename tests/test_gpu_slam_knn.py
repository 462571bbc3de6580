"""GPU: the statistical outlier filter and normals over the k nearest on the cloud of the SLAM driver - the tiny synthetic
run of tests/test_gpu_slam_cloud.py (TINY_CFG random weights on 128x256 frames, every keyframe overwritten in place with
keyframes that see one surface).  The new calls are applied to what SLAM.reconstruction returns.  What is checked: the
filter returns a subset in source order that is exactly the rows its own statistics select, every normal is unit length
or zero and faces the camera that saw its point, and the producer is as it was."""
import math

import pytest
import torch

from mast3r_slam import cloud, fusion, mast3r_utils
from test_gpu_slam_cloud import slam  # noqa: F401  (the fixture: the same run)

pytestmark = pytest.mark.gpu


def test_reconstruction_through_the_statistical_filter_and_knn_normals(slam):  # noqa: F811
    lo, hi = fusion.map_bounds(slam.keyframes)
    v = float((hi - lo).max()) / 128.0
    pts = slam.reconstruction(voxel_size=v, return_index=True)
    before = [t.clone() for t in pts]
    m = pts[0].shape[0]
    assert m > 1000
    k = 16
    out = mast3r_utils.remove_statistical_outliers(pts, k=k, std_ratio=2.0, radius=3 * v, return_rows=True, return_stats=True)
    assert len(out) == 5
    rows, st = out[3], out[4]
    assert 0 < rows.shape[0] < m and bool((rows[1:] > rows[:-1]).all())         # a subset in source order
    q = st["q"]
    nn = mast3r_utils.cloud_knn(pts[0], k, 3 * v)
    assert isinstance(nn, mast3r_utils.KnnResult) and nn.out_of_range == 0
    complete = nn.found == k
    assert torch.equal(q >= 0, complete) and st["n"] == int(complete.sum()) > m // 2
    assert st["S1"] == int(q[complete].to(torch.int64).sum()) and st["S2"] == sum(int(x) ** 2 for x in q[complete].tolist())
    assert st["T"] == cloud.statistical_threshold(st["n"], st["S1"], st["S2"], 2.0)
    assert torch.equal(rows, torch.nonzero(complete & (q <= math.floor(st["T"]))).reshape(-1))
    assert torch.equal(out[0], pts[0][rows]) and torch.equal(out[1], pts[1][rows]) and torch.equal(out[2], pts[2][rows])
    # q is the mean distance in units of r / (k 2^16): against dist2, to float32 accuracy
    mean = nn.dist2[complete].double().sqrt().mean(dim=1) / (3 * v)
    assert float((q[complete].double() / (k * 65536.0) - mean).abs().max()) <= 1e-4
    print(f"cloud: {m} points, {st['n']} complete at k = {k}, T = {st['T']:.1f}, {rows.shape[0]} kept")

    toward = mast3r_utils.source_viewpoints(slam.keyframes, pts[2])
    n, var = mast3r_utils.cloud_normals_knn(pts, 3 * v, k, toward=toward, return_variation=True)
    assert n.shape == (m, 3) and n.dtype == torch.float32 and var.shape == (m,)
    length = n.double().norm(dim=1)
    zero = ~n.any(dim=1)
    assert bool(((length - 1.0).abs() <= 1e-6)[~zero].all()) and bool((var[zero] == 0).all())
    to = toward.double() - pts[0].double()
    assert bool(((n.double() * to).sum(dim=1) >= -1e-6 * to.norm(dim=1))[~zero].all())
    assert bool(zero[nn.found + 1 < 3].all()) and int(zero.sum()) < m // 2      # below min_points: no normal
    assert torch.equal(mast3r_utils.cloud_normals_knn(pts, 3 * v, k, toward=toward), n)             # twice

    assert all(torch.equal(a, b) for a, b in zip(pts, before))                  # the inputs are as they were
    again = slam.reconstruction(voxel_size=v, return_index=True)
    assert all(torch.equal(a, b) for a, b in zip(again, before))                # the producer is as it was
