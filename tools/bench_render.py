"""Device time of render.render_map against what the parent commit offers (collect_map + a torch composition).

    python tools/bench_render.py [--out profiles/render_bench.json]

Events around `reps` graph replays (render) or eager calls (the torch yardstick, which synchronises inside collect_map);
median of `rounds` rounds.  Scenes: K keyframes of 512 x 512 (tests/render_scenes.general_scene), camera inside the map
and 400 units away (all points in a few pixels)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mast3r-slam_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import render_scenes as RS  # noqa: E402
from mast3r_slam import export, render  # noqa: E402


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


def torch_render(frames, view, Kc, size, thr):
    """The yardstick: exported cloud -> project -> packed key -> scatter_reduce(amin) -> gather (point_size 1)."""
    p, c, i = export.collect_map(frames, c_conf_threshold=thr, return_index=True)
    Hv, Wv = size
    T = view.double()
    x, y, z, w = T[3], T[4], T[5], T[6]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                     2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]).reshape(3, 3).float()
    cam = ((p - T[:3].float()) @ R) * (1.0 / T[7]).float()
    zc = cam[:, 2]
    px = torch.floor(Kc[0] * (cam[:, 0] / zc) + Kc[2] + 0.5)
    py = torch.floor(Kc[1] * (cam[:, 1] / zc) + Kc[3] + 0.5)
    ok = (zc > 0.5) & (px >= 0) & (px < Wv) & (py >= 0) & (py < Hv)
    pix = (py[ok].long() * Wv + px[ok].long())
    key = (zc[ok].view(torch.int32).long() << 32) | i[ok]
    keys = torch.full((Hv * Wv,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=p.device)
    keys.scatter_reduce_(0, pix, key, "amin")
    hit = keys != torch.iinfo(torch.int64).max
    src = torch.where(hit, keys & 0xffffffff, torch.zeros_like(keys))
    row = torch.searchsorted(i, src)
    rgb = torch.where(hit[:, None], c[row.clamp_max(c.shape[0] - 1)], torch.zeros_like(c[:1]))
    depth = torch.where(hit, (keys >> 32).int().view(torch.float32), torch.full((), float("inf"), device=p.device))
    return rgb.reshape(Hv, Wv, 3), depth.reshape(Hv, Wv), torch.where(hit, src, -torch.ones_like(src)).reshape(Hv, Wv)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--keyframes", default="16,256")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for K in [int(v) for v in a.keyframes.split(",")]:
        sc = RS.general_scene(K, 512, 512, seed=K, layout="u8")
        frames = RS.frames_of(sc, dev)
        tables = render.map_tables(frames)
        for size in ((480, 640), (1080, 1920)):
            inside, Kc = RS.general_view(size, "inside")
            far = inside.copy()
            far[2] -= 400.0
            for where, v in (("inside", inside), ("far", far)):
                pose = torch.from_numpy(v).to(dev)
                for ps in (1, 3):
                    for thr in (1.5, None):
                        out = (torch.empty((*size, 3), dtype=torch.uint8, device=dev), torch.empty(size, dtype=torch.float32, device=dev),
                               torch.empty(size, dtype=torch.int64, device=dev))
                        ws = torch.empty(render.workspace_bytes(size), dtype=torch.uint8, device=dev)
                        call = lambda: render.render_map(tables, pose, Kc, size, near=0.5, c_conf_threshold=thr, point_size=ps,
                                                         return_index=True, out=out, workspace=ws)
                        call()
                        torch.cuda.synchronize()
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g):
                            call()
                        g.replay()
                        torch.cuda.synchronize()
                        ms = timed(g.replay, 20)
                        row = dict(K=K, size=list(size), camera=where, point_size=ps, thr=thr, render_ms=ms,
                                   covered=int((out[2] >= 0).sum()))
                        if ps == 1:
                            ref = torch_render(frames, pose, Kc, size, thr)
                            row["index_equal_to_torch"] = bool(torch.equal(ref[2], out[2]))
                            row["torch_ms"] = timed(lambda: torch_render(frames, pose, Kc, size, thr), 3, rounds=3)
                            row["ratio"] = row["torch_ms"] / ms
                        # bytes the call has to move at least: C of every point, X of the passing ones, keys twice, outputs
                        n = K * 512 * 512
                        passing = n if thr is None else int(sum(int(((f.C.reshape(-1) / f.N) > thr).sum()) for f in frames))
                        row["min_bytes"] = n * 4 + passing * 12 + size[0] * size[1] * (8 + 8 + 3 + 4 + 8)
                        row["tb_per_s"] = row["min_bytes"] / (ms * 1e-3) / 1e12
                        rows.append(row)
                        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
