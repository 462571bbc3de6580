#!/usr/bin/env python3
"""Lens undistortion on the device (camera.undistort_device, k_remap_bilinear): kernel time, share of the HBM rate, the
torch.grid_sample yardstick and the cost inside Dataset.frames, in one process on one box.

    python tools/bench_undistort.py [--out profiles/undistort_bench.md] [--no-pair]

Kernel time: device events around one replay of a hipGraph that holds 20 launches, warmed.  The A/B against the staged
experiment (tools/experiments/undistort_staged.hip) alternates the two graphs round by round in this process.  The
batch-1 tracking step is measured here too (the full network at 512x512 on one pair, matching and Gauss-Newton
tracking, graph-replayed: the step bench.py reports as batch1.ms_per_pair); --no-pair skips it.  Registers, LDS and
scratch come from compiling the two sources with -Rpass-analysis=kernel-resource-usage.
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mast3r-slam_amd"), os.path.join(ROOT, "tools", "experiments")]
import numpy as np
import torch

import undistort_staged as staged
from mast3r_slam import camera, dataloader, synthetic

HBM_PEAK_TBS = 8.0                             # MI355X HBM3E peak
HBM_COPY_TBS = 6.29                            # the rate a float4 copy kernel reaches on it
AB_ROUNDS = 7
CASES = [(480, 640), (720, 1280), (1080, 1920)]
DIST = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)       # a wide-angle radtan lens, K scaled to each size
LAUNCHES = 20


def make_camera(h, w):
    return camera.CameraModel(w, h, [458.654 * w / 752, 457.296 * h / 480, 367.215 * w / 752, 248.375 * h / 480], DIST, "radtan")


def med(v):
    return statistics.median(v), min(v), max(v)


def fmt(v, unit=1.0):
    m, lo, hi = med(v)
    return f"{m * unit:.3f} ({lo * unit:.3f} - {hi * unit:.3f})"


def resource_usage(src=os.path.join(ROOT, "mast3r-slam_amd", "csrc", "undistort.hip")):
    """VGPRs, SGPRs, LDS and scratch of the one kernel in `src` as the compiler reports them."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-c", src, "-o", os.path.join(d, "u.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    if r.returncode != 0:
        return None
    get = lambda key: int(re.search(key + r"[^:]*: (\d+)", r.stderr).group(1))
    return {"vgpr": get("VGPRs"), "sgpr": get("TotalSGPRs"), "lds": get("LDS Size"), "scratch": get("ScratchSize"),
            "occupancy": get("Occupancy")}


def usage_text(u):
    return (f"{u['vgpr']} VGPRs, {u['sgpr']} SGPRs, {u['lds']} bytes of LDS, {u['scratch']} bytes of scratch per lane, "
            f"occupancy {u['occupancy']} waves per SIMD" if u else "not measured (hipcc did not run)")


def make_graph(call):
    """A warmed hipGraph of LAUNCHES captured calls."""
    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(LAUNCHES):
            call()
    g.replay()
    torch.cuda.synchronize()
    return g


def replay_time(g, reps):
    """us per captured call, `reps` timed replays."""
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); g.replay(); e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) / LAUNCHES * 1e3)
    return t


def alternating_ab(call_a, call_b, reps):
    """AB_ROUNDS rounds of (A, B): the median of `reps` replays of each per round -> (medians of A, medians of B)."""
    ga, gb = make_graph(call_a), make_graph(call_b)
    ta, tb = [], []
    for _ in range(AB_ROUNDS):
        ta.append(statistics.median(replay_time(ga, reps)))
        tb.append(statistics.median(replay_time(gb, reps)))
    return ta, tb


def batch1_pair_ms(dev):
    """ms of one batch-1 tracking step, graph-replayed: the full network on one 512x512 pair, matching, the
    10-iteration pose solve - the three legs of bench.py's pairs workload with one pair (its batch1.ms_per_pair)."""
    from types import SimpleNamespace

    import bench
    args = bench.parse(["--pairs-per-gpu", "1"])
    wl = bench.PairsWorkload(args, SimpleNamespace(rank=0, world=1, local=0, dev=dev, dist=None, group=None))

    def step():
        o = wl.leg_infer()
        idx, valid = wl.leg_match()
        return o, wl.leg_gn(idx, valid)
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = step()           # noqa: F841 - the graph's static outputs
    g.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        g.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / 10 * 1e3


def graph_time(call, reps):
    """us per call: events around a replay of LAUNCHES captured calls."""
    return replay_time(make_graph(call), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undistort_bench.md"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-pair", action="store_true", help="skip the batch-1 tracking step (the full network)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_undistort needs a ROCm device")
    dev = torch.device("cuda:0")
    usage = resource_usage()
    if usage is not None and usage["scratch"] != 0:
        raise SystemExit(f"k_remap_bilinear spills to scratch: {usage}")
    usage_staged = resource_usage(staged.SRC)
    krows, frows, abrows, wall_rows = [], [], [], []
    for h, w in CASES:
        cam = make_camera(h, w)
        tab = torch.from_numpy(cam.undistort_table("inner").copy()).to(dev)
        # the yardstick's sampling grid: the same coordinates, normalised for grid_sample (align_corners=True)
        grid = tab.to(torch.float32) / 256.0
        grid = torch.stack([grid[..., 0] * 2 / (w - 1) - 1, grid[..., 1] * 2 / (h - 1) - 1], -1)
        for batch in (1, 8):
            frames = np.stack([synthetic.textured_image(h, w, s) for s in range(batch)])
            src = torch.from_numpy(frames).to(dev)
            kt = graph_time(lambda: camera.remap_bilinear(src, tab), a.reps)
            gb = grid[None].expand(batch, -1, -1, -1)

            def yardstick():
                f = src.permute(0, 3, 1, 2).to(torch.float32)
                o = torch.nn.functional.grid_sample(f, gb, mode="bilinear", padding_mode="zeros", align_corners=True)
                return (o + 0.5).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

            yt = graph_time(yardstick, a.reps)
            ours, theirs = camera.remap_bilinear(src, tab), yardstick()
            off = int((ours.to(torch.int16) - theirs.to(torch.int16)).abs().max())
            # algorithmic bytes: the table once (the batch shares it), each frame's source and output once
            nbytes = h * w * 8 + batch * h * w * 6
            us = med(kt)[0]
            tbs = nbytes / us / 1e6
            krows.append(f"| {w}x{h} | {batch} | {fmt(kt)} | {nbytes / 1e6:.2f} | {tbs:.3f} | {tbs / HBM_PEAK_TBS:.3f} | "
                         f"{tbs / HBM_COPY_TBS:.3f} | {fmt(yt)} | {med(yt)[0] / us:.1f}x | {off} |")
            if (h, w) == (1080, 1920):
                # the A/B: same table, same frames, the two graphs replayed in alternation
                boxes_h = staged.tile_boxes(tab.cpu().numpy(), h, w)
                boxes = torch.from_numpy(boxes_h).to(dev)
                if not torch.equal(staged.remap_staged(src, tab, boxes), ours):
                    raise SystemExit("the staged kernel's bytes differ from the library's")
                ta, tb = alternating_ab(lambda: camera.remap_bilinear(src, tab), lambda: staged.remap_staged(src, tab, boxes), a.reps)
                ma, mb = statistics.median(ta), statistics.median(tb)
                spread = max(max(ta) - min(ta), max(tb) - min(tb))
                verdict = "staged faster" if ma - mb > spread else ("baseline faster" if mb - ma > spread else "within the spread")
                abrows.append(f"| {w}x{h} | {batch} | {fmt(ta)} | {fmt(tb)} | {ma - mb:+.3f} | {spread:.3f} | "
                              f"{staged.staged_share(boxes_h):.3f} | {verdict} |")
        # Dataset.frames per frame, batch 1, with and without the calibration (upload + launches + a synchronise per frame)
        raw = [synthetic.textured_image(h, w, s) for s in range(8)]
        wall = {}
        for name, ds in (("plain", dataloader.ArrayDataset(raw)), ("calibrated", dataloader.ArrayDataset(raw, calibration=cam))):
            def run():
                for _, f in ds.frames(dev):
                    pass
                torch.cuda.synchronize()
            run()
            t = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                run()
                t.append((time.perf_counter() - t0) * 1e3 / len(raw))
            wall[name] = t
        wall_rows.append((f"{w}x{h}", wall))
    ms_pair = None if a.no_pair else batch1_pair_ms(dev)
    for shape, wall in wall_rows:
        extra = med(wall["calibrated"])[0] - med(wall["plain"])[0]
        share = f"{extra / ms_pair:.4f}" if ms_pair else "not measured"
        frows.append(f"| {shape} | {fmt(wall['plain'])} | {fmt(wall['calibrated'])} | {extra:.3f} | {share} |")
    pair = f"{ms_pair:.3f} ms (this process)" if ms_pair else "not measured"
    res = usage_text(usage)
    txt = f"""# Lens undistortion (tools/bench_undistort.py)

Box: {torch.cuda.get_device_name(0)}; {a.reps} repetitions, median (min - max).  Frames: `synthetic.textured_image`; camera: a radtan
lens {DIST} with K scaled to each size, `K_new = "inner"`, output size = source size.

`k_remap_bilinear` as compiled for gfx950: {res}.

Kernel alone (source and table on the device): device events around one replay of a hipGraph of {LAUNCHES} launches, per launch.
Algorithmic bytes = the table once (8 per pixel, shared by the batch) + source and output once per frame (3 + 3 per
pixel), as a share of the HBM peak ({HBM_PEAK_TBS} TB/s) and of what a float4 copy reaches ({HBM_COPY_TBS} TB/s).  Yardstick in the same process:
`torch.nn.functional.grid_sample` (bilinear, zero padding) over a float copy of the same frames on the device, with the
conversion to float32 NCHW and back to uint8 NHWC - what a user would write today.  It rounds differently (last column:
the largest difference in grey levels), so it is a yardstick of time only.

| shape | batch | remap us/launch | MB moved | TB/s | of peak | of copy rate | grid_sample us | grid_sample / remap | max grey-level difference |
|---|---|---|---|---|---|---|---|---|---|
{chr(10).join(krows)}

A/B against the staged experiment (`tools/experiments/undistort_staged.hip`: a 64 x 4 tile's source box copied to LDS with
16-byte loads, taps read from LDS; {usage_text(usage_staged)}).  Same bytes (checked here).  {AB_ROUNDS} rounds of
baseline, staged, baseline, staged ...; each round's figure is the median of {a.reps} graph replays; the table shows the
median (min - max) over the rounds, spread = the larger max - min of the two.  The staged kernel would ship only if it
were faster by more than the spread.

| shape | batch | baseline us | staged us | baseline - staged us | spread us | tiles staged | verdict |
|---|---|---|---|---|---|---|---|
{chr(10).join(abrows)}

`Dataset.frames` per frame at batch 1 (host clock; upload, launches and the consumer's synchronise included), without
and with a calibration.  Batch-1 tracking step (network pair, matching, pose solve; graph replay): {pair}.

| source | frames() ms/frame | calibrated frames() ms/frame | added ms/frame | added / ms_per_pair |
|---|---|---|---|---|
{chr(10).join(frows)}
"""
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt)
    print(txt)


if __name__ == "__main__":
    main()
