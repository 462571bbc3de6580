#!/usr/bin/env python3
"""Frame preprocessing: the host path (mast3r_utils.resize_img with PIL, then the upload of its network-sized result)
against the device path (upload of the raw frame, then resize_img_device), in one process on one box.

    python tools/bench_preprocess.py [--out profiles/preprocess_bench.md] [--ms-per-pair MS] [--launch-floor-us US]

Wall time per frame ends in a device synchronise on both sides.  Device time is taken with events behind queued work
(the launches of a whole repetition are queued before the first one is waited for).  `--ms-per-pair`: the batch-1
tracking step of the same box (bench.py --full, "ms_per_pair"), `--launch-floor-us`: tools/launch_floor.py's figure.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mast3r-slam_amd")]
import numpy as np
import torch

from mast3r_slam import mast3r_utils, preprocess, synthetic

HBM_TBS = 8.0
CASES = [(480, 640), (720, 1280), (1080, 1920)]


def med(v):
    return statistics.median(v), min(v), max(v)


def fmt(v, unit=1.0):
    m, lo, hi = med(v)
    return f"{m * unit:.3f} ({lo * unit:.3f} - {hi * unit:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess_bench.md"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ms-per-pair", type=float, default=None)
    ap.add_argument("--launch-floor-us", type=float, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_preprocess needs a ROCm device")
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    rows, krows = [], []
    for h, w in CASES:
        for batch in (1, 8):
            frames = np.stack([synthetic.textured_image(h, w, s) for s in range(batch)])
            pinned = torch.from_numpy(frames).pin_memory()
            (W, H), kind, box, _ = preprocess.resize_geometry(h, w, 512)
            hc, wc = box[3] - box[1], box[2] - box[0]

            def host():
                for f in frames:
                    torch.from_numpy(mast3r_utils.resize_img(f, 512)["unnormalized_img"]).to(dev)
                sync()

            def device_pageable():
                preprocess.resize_img_device(torch.from_numpy(frames).to(dev))
                sync()

            def device_pinned():
                preprocess.resize_img_device(pinned.to(dev, non_blocking=True))
                sync()

            def upload_only():
                torch.from_numpy(frames).to(dev)
                sync()

            wall = {}
            for name, fn in (("host", host), ("pageable", device_pageable), ("pinned", device_pinned), ("upload", upload_only)):
                fn(); fn()
                t = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    fn()
                    t.append((time.perf_counter() - t0) * 1e3 / batch)
                wall[name] = t
            # the kernel alone: device events, 10 queued launches per repetition, source already on the device
            src = torch.from_numpy(frames).to(dev)
            call = lambda: preprocess.resize_crop(src, (W, H), kind, box)
            call(); sync()
            kt = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(10):
                    call()
                e1.record(); sync()
                kt.append(e0.elapsed_time(e1) / 10 * 1e3)                      # us per call
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(10):
                    call()
            g.replay(); sync()
            gt = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); g.replay(); e1.record(); sync()
                gt.append(e0.elapsed_time(e1) / 10 * 1e3)
            # algorithmic bytes: the source rows and columns under the crop box once, uint8 + float32 outputs once
            nbytes = batch * (h * w * 3 + hc * wc * 3 * 5)
            us = med(gt)[0]
            ratio = med(wall["host"])[0] / med(wall["pageable"])[0]
            rows.append(f"| {w}x{h} | {batch} | {fmt(wall['host'])} | {fmt(wall['pageable'])} | {fmt(wall['pinned'])} | "
                        f"{ratio:.2f}x | {fmt(wall['upload'])} | {med(wall['upload'])[0] / med(wall['pageable'])[0]:.2f} |")
            extra = f" {us / batch / 1e3 / a.ms_per_pair:.4f} |" if a.ms_per_pair else " not measured |"
            krows.append(f"| {w}x{h} -> {wc}x{hc} | {batch} | {fmt(kt)} | {fmt(gt)} | {nbytes / 1e6:.2f} | "
                         f"{nbytes / us / 1e6 / HBM_TBS:.3f} | {nbytes / 1e6 / HBM_TBS:.2f} |{extra}")
    name = torch.cuda.get_device_name(0)
    floor = f"{a.launch_floor_us:.2f} us per launch (tools/launch_floor.py, same box)" if a.launch_floor_us else "not measured here"
    pair = f"{a.ms_per_pair:.3f} ms (bench.py, same box)" if a.ms_per_pair else "not measured here"
    txt = f"""# Frame preprocessing (tools/bench_preprocess.py)

Box: {name}; {a.reps} repetitions, median (min - max).  Frames: `synthetic.textured_image`, target size 512.  Wall times are
per frame, host clock around work that ends in a device synchronise.  Host path = the parent commit's: `resize_img` (PIL
LANCZOS + crop + normalise) per frame, then the upload of its uint8 result.  Device path = upload of the raw frame(s)
(pageable numpy memory, or a pinned tensor) + one `resize_img_device` call for the batch.

| source | batch | host path ms/frame | device path ms/frame (pageable) | device path ms/frame (pinned) | host / device | raw upload alone ms/frame | upload share of the device path |
|---|---|---|---|---|---|---|---|
{chr(10).join(rows)}

Kernel alone (`k_resize_crop`, source already on the device; uint8 and float32 outputs): device events around 10 queued
`resize_crop` calls (one launch each), eager and replayed from a hipGraph.
Algorithmic bytes = source once + both outputs once; HBM reference {HBM_TBS} TB/s; byte floor = those bytes at that rate.
Launch floor: {floor}.  Batch-1 tracking step: {pair}.

| shape | batch | eager us/call | graph us/call | MB moved | of HBM (graph) | byte floor us | device time per frame / ms_per_pair |
|---|---|---|---|---|---|---|---|
{chr(10).join(krows)}
"""
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt)
    print(txt)


if __name__ == "__main__":
    main()
