"""Device time of consistency.multiview_support against the same rule composed from torch operations.

    python tools/bench_consistency.py [--out profiles/consistency_bench.md] [--keyframes 16,256] [--neighbours 8]

K keyframes of 512 x 512 that see one surface (tests/consistency_twin.shared_scene), threshold 1.5, the V nearest camera
centres as neighbours, the default rule.  Events around `reps` graph replays after a warm-up, median of 5 rounds; the
HIP path is also timed eagerly on prebuilt tables.  The yardstick is the rule in fp32 torch operations in the same
process, on inputs that are already stacked ([K,N,3], [K,N]: a layout the map does not have, the copy is not charged):
the observation planes and world points batched over the keyframes, then per neighbour pair (k, j) the act into j's
frame, the projection and one index gather, with no host synchronisation inside (the neighbour table is read back once,
before the clock starts).  Algorithmic traffic of the HIP path: the plane pass reads X and C and writes D (20 bytes per
point), the count pass reads X and C and writes two counts and the masked confidence (22 bytes per point) and gathers
at most V depths of 4 bytes per point: K N (42 + 4 V) bytes."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mast3r-slam_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import consistency_twin as CT  # noqa: E402
import render_scenes as RS  # noqa: E402
from mast3r_slam import _ffi, consistency, render  # noqa: E402

H = W = 512
THR, Z_MIN, RTOL, MIN_VIEWS, MAX_CONFLICTS = 1.5, 1e-3, 0.03, 2, 1


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


def torch_rule(X, C, nk, T, pin, nbr_rows):
    """The yardstick: X float32 [K,N,3], C float32 [K,N], nk float32 [K,1], T float32 [K,8], nbr_rows a host list of
    lists -> (support uint8 [K,N], conflict uint8 [K,N], conf float32 [K,N])."""
    fx, fy, cx, cy = pin
    K, N = C.shape
    passes = (C / nk) > THR
    z = X[..., 2]
    D = torch.where(passes & torch.isfinite(z) & (z > Z_MIN), z, torch.full_like(z, float("nan")))
    t, q, s = T[:, None, :3], T[:, None, 3:7], T[:, None, 7:8]
    qv, w = q[..., :3].expand(K, N, 3), q[..., 3:4]
    u = 2.0 * torch.linalg.cross(qv, X)
    world = s * (X + w * u + torch.linalg.cross(qv, u)) + t
    cand = passes & torch.isfinite(world).all(dim=2)
    x_, y_, z_, w_ = (T[:, i].double() for i in (3, 4, 5, 6))
    R = torch.stack([1 - 2 * (y_ * y_ + z_ * z_), 2 * (x_ * y_ - w_ * z_), 2 * (x_ * z_ + w_ * y_),
                     2 * (x_ * y_ + w_ * z_), 1 - 2 * (x_ * x_ + z_ * z_), 2 * (y_ * z_ - w_ * x_),
                     2 * (x_ * z_ - w_ * y_), 2 * (y_ * z_ + w_ * x_), 1 - 2 * (x_ * x_ + y_ * y_)], dim=1).reshape(K, 3, 3).float()
    inv_s = (1.0 / T[:, 7].double()).float()
    support = torch.zeros((K, N), dtype=torch.uint8, device=X.device)
    conflict = torch.zeros((K, N), dtype=torch.uint8, device=X.device)
    for k, row in enumerate(nbr_rows):
        for j in row:
            if j < 0 or j >= K or j == k:
                continue
            c = ((world[k] - T[j, :3]) @ R[j]) * inv_s[j]                       # R_j^T (p - t_j) / s_j
            cz = c[:, 2]
            px = torch.floor(fx * (c[:, 0] / cz) + cx + 0.5)
            py = torch.floor(fy * (c[:, 1] / cz) + cy + 0.5)
            inside = cand[k] & (cz > Z_MIN) & (px >= 0) & (px < W) & (py >= 0) & (py < H)
            pix = torch.where(inside, py * W + px, torch.zeros_like(px)).long()
            d = D[j][pix]
            seen = inside & ~torch.isnan(d)
            agree = seen & ((cz - d).abs() <= RTOL * d)
            support[k] += agree
            conflict[k] += seen & ~agree & (cz < d)
    kept = cand & (support >= MIN_VIEWS) & (conflict <= MAX_CONFLICTS)
    return support, conflict, torch.where(kept, C, torch.full_like(C, float("-inf")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consistency_bench.md"))
    ap.add_argument("--keyframes", default="16,256")
    ap.add_argument("--neighbours", type=int, default=8)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    pin = CT.shared_pinhole(H, W)
    rows = []
    for K in [int(v) for v in a.keyframes.split(",")]:
        sc = CT.shared_scene(K, H, W, seed=K)
        frames = RS.frames_of(sc, dev)
        del sc["img"]
        tables = render.map_tables(frames)
        nbr = consistency.nearest_neighbours(tables.poses, a.neighbours)
        V = int(nbr.shape[1])
        out = (torch.empty((K, H * W), dtype=torch.uint8, device=dev), torch.empty((K, H * W), dtype=torch.uint8, device=dev),
               torch.empty((K, H * W), dtype=torch.float32, device=dev))
        ws = torch.empty(consistency.workspace_bytes(K, H * W), dtype=torch.uint8, device=dev)
        call = lambda: consistency.multiview_support(tables, pin, neighbours=nbr, out=out, workspace=ws)
        call()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        g.replay()
        torch.cuda.synchronize()
        reps = max(2, 128 // K)
        row = dict(K=K, V=V, size=[H, W], launches=int(_ffi.lib().m3_consistency_launches()), hip_graph_ms=timed(g.replay, reps),
                   hip_eager_ms=timed(call, reps))
        Xs, Cs = torch.stack([f.X_canon for f in frames]), torch.stack([f.C.reshape(-1) for f in frames])
        nk = torch.tensor([[float(f.N)] for f in frames], dtype=torch.float32, device=dev)
        nbr_rows = nbr.cpu().tolist()
        ref = torch_rule(Xs, Cs, nk, tables.poses, pin, nbr_rows)
        torch.cuda.synchronize()
        row["torch_ms"] = timed(lambda: torch_rule(Xs, Cs, nk, tables.poses, pin, nbr_rows), 1, rounds=3)
        row["ratio"] = row["torch_ms"] / row["hip_graph_ms"]
        pairs = K * H * W * V
        row["pairs"] = pairs
        row["support_differs"] = int((ref[0] != out[0]).sum())
        row["conflict_differs"] = int((ref[1] != out[1]).sum())
        row["kept"] = int((out[2] > float("-inf")).sum())
        row["candidates"] = int(((Cs / nk) > THR).sum())
        row["algorithmic_bytes"] = K * H * W * (42 + 4 * V)
        row["tb_per_s"] = row["algorithmic_bytes"] / (row["hip_graph_ms"] * 1e-3) / 1e12
        row["gpairs_per_s"] = pairs / (row["hip_graph_ms"] * 1e-3) / 1e9
        rows.append(row)
        print(json.dumps(row), flush=True)
        del Xs, Cs, ref, frames, tables, out, ws, g
        torch.cuda.empty_cache()
    lines = ["# Multi-view consistency filter: `consistency.multiview_support` against the rule in torch operations", "",
             "Tool: `python tools/bench_consistency.py` (its docstring says what is timed and how the traffic is counted).  "
             f"Device: {torch.cuda.get_device_name(0)}.", "",
             "| K | V | pairs | HIP, graph replay (ms) | HIP, eager (ms) | torch fp32 (ms) | torch / HIP | algorithmic TB/s | 10^9 pairs/s | "
             "sources whose support / conflict differs from torch | kept of candidates |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['K']} | {r['V']} | {r['pairs']:.3g} | {r['hip_graph_ms']:.3f} | {r['hip_eager_ms']:.3f} | {r['torch_ms']:.1f} | "
                     f"{r['ratio']:.0f} | {r['tb_per_s']:.2f} | {r['gpairs_per_s']:.1f} | {r['support_differs']} / {r['conflict_differs']} | "
                     f"{r['kept']} of {r['candidates']} |")
    lines += ["", "`pairs` is K N V; only candidates are projected (the `kept of candidates` column gives their number), so the "
              "gathers move less than the 4 V bytes per point the algorithmic figure charges: it is an upper bound on the "
              "traffic and the TB/s column an upper bound on the rate.  16 keyframes (67 MB of inputs and planes) fit the 256 "
              "MiB Infinity Cache, so a replay loop at that size measures cache bandwidth; 256 keyframes (1.3 GB) do not.  "
              "The torch column makes about 25 launches per neighbour pair on 262144 points each.  A count differs from "
              "torch where the two world points differ in the last bit (torch does not fuse `act` as the exporter's "
              "kernel does) at a contested pair; no counter run was made, so nothing here says what binds `k_cons_count`.",
              "", "```json", json.dumps(rows), "```", ""]
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
