"""Device time of intrinsics.estimate_focal against the same formula written with torch float64 operations.

    python tools/bench_focal.py [--out profiles/intrinsics_bench.json] [--keyframes 1,16,128] [--iters 10]

K keyframes of 512 x 512 from the recipe of tests/focal_twin.py (four distinct keyframes, repeated in separate device
buffers), threshold 1.5.  Events around `reps` calls after a warm-up, median of `rounds` rounds.  The HIP path is timed
eagerly on prebuilt tables and as a graph replay; the yardstick gets its inputs already stacked ([K,N,3] and [K,N]
device tensors, which the map does not have: the stacking copy is not charged to it), is batched over the keyframes
and makes no host synchronisation.  Algorithmic traffic: every pass reads X and C once, (iters + 2) K N 16 bytes."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mast3r-slam_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import focal_twin as FT  # noqa: E402
import render_scenes as RS  # noqa: E402
from mast3r_slam import _ffi, intrinsics, render  # noqa: E402

H = W = 512


def timed(fn, reps, rounds=5):
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return float(np.median(out))


def torch_focal(X, C, nk, thr, cx, cy, z_min, iters):
    """The yardstick: X float32 [K,N,3], C float32 [K,N], nk float32 [K,1] -> float64 [K,4], the rule of
    include/m3slam.h in torch operations."""
    n = torch.arange(X.shape[1], device=X.device)
    u, v = (n % W).double() - cx, (n // W).double() - cy
    ok = torch.isfinite(X).all(dim=2) & (X[..., 2] > z_min) & ((C / nk) > thr)
    x, y, z = X[..., 0].double(), X[..., 1].double(), X[..., 2].double()
    a, b = x / z, y / z
    zero = torch.zeros((), dtype=torch.float64, device=X.device)
    pq, qq = torch.where(ok, a * u + b * v, zero), torch.where(ok, a * a + b * b, zero)
    a, b = torch.where(ok, a, zero), torch.where(ok, b, zero)
    f0 = f = pq.sum(dim=1) / qq.sum(dim=1)

    def dist(f):
        du, dv = u - f[:, None] * a, v - f[:, None] * b
        return torch.sqrt(du * du + dv * dv)

    for _ in range(iters):
        w = 1.0 / dist(f).clamp_min(1e-8)
        f = (w * pq).sum(dim=1) / (w * qq).sum(dim=1)
    count = ok.sum(dim=1).double()
    return torch.stack([f, f0, count, torch.where(ok, dist(f), zero).sum(dim=1) / count], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--keyframes", default="1,16,128")
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    base = FT.pinhole_scene(H, W, [400.0, 520.0, 450.0, 610.0], seed=1, nks=[1, 2, 3, 1])
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    rows = []
    for K in [int(v) for v in a.keyframes.split(",")]:
        pick = [k % base["K"] for k in range(K)]
        sc = dict(base, X=base["X"][pick], C=base["C"][pick], Nk=base["Nk"][pick], T=base["T"][pick], img=base["img"][pick], K=K)
        frames = RS.frames_of(sc, dev)
        tables = render.map_tables(frames)
        out = torch.empty((K, 4), dtype=torch.float64, device=dev)
        ws = torch.empty(intrinsics.workspace_bytes(K, H * W), dtype=torch.uint8, device=dev)
        call = lambda: intrinsics.estimate_focal(tables, iters=a.iters, out=out, workspace=ws)
        call()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        g.replay()
        torch.cuda.synchronize()
        reps = max(3, 200 // K)
        row = dict(K=K, size=[H, W], iters=a.iters, launches=int(_ffi.lib().m3_focal_launches(a.iters)),
                   hip_graph_ms=timed(g.replay, reps), hip_eager_ms=timed(call, reps))
        Xs, Cs = torch.stack([f.X_canon for f in frames]), torch.stack([f.C.reshape(-1) for f in frames])
        nk = torch.tensor([[float(f.N)] for f in frames], dtype=torch.float32, device=dev)
        ref = torch_focal(Xs, Cs, nk, 1.5, cx, cy, 0.0, a.iters)
        torch.cuda.synchronize()
        row["torch_ms"] = timed(lambda: torch_focal(Xs, Cs, nk, 1.5, cx, cy, 0.0, a.iters), max(2, 20 // K), rounds=3)
        row["ratio"] = row["torch_ms"] / row["hip_graph_ms"]
        row["max_rel_diff_to_torch"] = float(((out - ref).abs() / ref.abs()).max())
        row["focal_first_rows"] = out[:4, 0].tolist()
        row["algorithmic_bytes"] = (a.iters + 2) * K * H * W * 16
        row["tb_per_s"] = row["algorithmic_bytes"] / (row["hip_graph_ms"] * 1e-3) / 1e12
        rows.append(row)
        print(json.dumps(row), flush=True)
        del Xs, Cs, ref
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
