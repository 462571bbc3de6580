"""Device time of the volumetric fusion: fusion.fuse_tsdf and fusion.extract_surface on 512 x 512 keyframes.

    python tools/bench_tsdf.py [--out profiles/tsdf_bench.md] [--cases 256:16,512:64] [--stats 256:16=DIR,512:64=DIR]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_tsdf.py --workload --cases 256:16

A case D:K is a cube of D^3 voxels over K keyframes of 512 x 512 that see one surface (tests/consistency_twin.
shared_scene), threshold 1.5: the cube [-2, 2] x [-2, 2] x [0.5, 4.5] holds the tilted plane every keyframe sees and the
free space in front of it, voxel size 4 / D, trunc 4 voxels.  Call times: device events around `reps` eager calls on
prebuilt tables, out and workspace (nothing is read back) after a warm-up, median of 5 rounds, for the integration; a
host clock around calls that end in the extraction's own synchronising read of V and F, for the extraction.  Kernel
times come from a separate run of `--workload` (the same calls, untimed) under rocprofv3, whose output directory is
given with --stats; without it the kernel table says "not measured".

What the kernels have to move, from the shapes alone: the voxel kernel writes 4 + 4 + 3 + 1 bytes per voxel and makes up
to K gathers of 4 bytes (and of a colour) per voxel, D^3 K voxel-keyframe pairs of arithmetic; the extraction reads
tsdf and weight once (8 bytes per voxel) and writes one flag byte in the cell pass, reads the flag byte in each of the
three later passes and the remap where an edge yields faces, and writes 15 bytes per vertex, 4 per remap entry and 12
per face: 12 D^3 + 19 V + 28 F bytes."""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mast3r-slam_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import consistency_twin as CT  # noqa: E402
import render_scenes as RS  # noqa: E402
from mast3r_slam import _ffi, fusion, render  # noqa: E402

H = W = 512
ORIGIN, SIDE = (-2.0, -2.0, 0.5), 4.0
HBM_PEAK = 8.0e12
YARDSTICK = (5.4e8, 1.387e-3)                  # k_cons_count: pairs, seconds (profiles/consistency_bench.md, 256 keyframes)


def event_ms(fn, reps, rounds=5):
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return float(np.median(out)), float(min(out)), float(max(out))


def host_ms(fn, reps, rounds=5):
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / reps)
    return float(np.median(out)), float(min(out)), float(max(out))


def kernel_stats(dirname):
    """{kernel name: (calls, average ns)} of the tsdf / scan / plane kernels in a rocprofv3 --stats directory."""
    hits = sorted(glob.glob(os.path.join(dirname, "**", "*kernel_stats.csv"), recursive=True))
    if not hits:
        raise SystemExit(f"no *kernel_stats.csv under {dirname}")
    out = {}
    for r in csv.DictReader(open(hits[0])):
        for key in ("k_tsdf_voxels", "k_tsdf_cells", "k_tsdf_count_edges", "k_tsdf_vertices", "k_tsdf_faces", "k_scan_counts",
                    "k_cons_plane", "k_cons_inverse"):
            if key in r["Name"]:
                out[key] = (int(r["Calls"]), float(r["AverageNs"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_bench.md"))
    ap.add_argument("--cases", default="256:16,512:64")
    ap.add_argument("--stats", default="")
    ap.add_argument("--workload", action="store_true", help="run the calls untimed (for a profiler) and write nothing")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: nothing is measured without one")
    dev = torch.device("cuda:0")
    stats = dict(kv.split("=") for kv in a.stats.split(",") if kv)
    pin = CT.shared_pinhole(H, W)
    L = _ffi.lib()
    rows = []
    for case in a.cases.split(","):
        D, K = (int(v) for v in case.split(":"))
        sc = CT.shared_scene(K, H, W, seed=K)
        frames = RS.frames_of(sc, dev)
        tables = render.map_tables(frames)
        vs = SIDE / D
        out = fusion.empty_volume(ORIGIN, (D, D, D), vs, device=dev)
        ws = torch.empty(fusion.workspace_bytes(K, H * W), dtype=torch.uint8, device=dev)
        fuse = lambda: fusion.fuse_tsdf(tables, pin, vs, out=out, workspace=ws)
        extract = lambda: fusion.extract_surface(out)
        fuse()
        v, _, f = extract()
        torch.cuda.synchronize()
        reps = max(2, (1 << 28) // (D ** 3 * K) * 4)
        if a.workload:
            for _ in range(3):
                fuse()
                extract()
            torch.cuda.synchronize()
            continue
        again = fusion.fuse_tsdf(tables, pin, vs, out=fusion.empty_volume(ORIGIN, (D, D, D), vs, device=dev), workspace=ws)
        same = all(torch.equal(x, y) for x, y in ((out.tsdf, again.tsdf), (out.weight, again.weight), (out.color, again.color)))
        del again
        row = dict(case=case, voxels=D ** 3, K=K, pairs=D ** 3 * K, V=int(v.shape[0]), F=int(f.shape[0]),
                   observed=float((out.weight > 0).float().mean()), identical_bytes=bool(same),
                   integrate_ms=event_ms(fuse, reps), extract_ms=host_ms(extract, max(2, reps // 2)),
                   integrate_launches=int(L.m3_tsdf_integrate_launches()), extract_launches=int(L.m3_tsdf_extract_launches()),
                   extract_bytes=12 * D ** 3 + 19 * int(v.shape[0]) + 28 * int(f.shape[0]))
        row["kernels"] = kernel_stats(stats[case]) if case in stats else None
        rows.append(row)
        print(json.dumps(row), flush=True)
        del frames, tables, out, ws, v, f
        torch.cuda.empty_cache()
    if a.workload:
        return
    lines = ["# Volumetric fusion: `fusion.fuse_tsdf` and `fusion.extract_surface`", "",
             "Tool: `python tools/bench_tsdf.py` (its docstring says what is timed and how the traffic is counted).  "
             f"Device: {torch.cuda.get_device_name(0)}.  Nothing here is a gate.", "",
             "| case (D:K) | voxel-keyframe pairs | observed voxels | V | F | integrate, eager call (ms: median, min, max) | "
             "extract, call with its host read (ms: median, min, max) | two integrations give identical bytes |",
             "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['pairs']:.3g} | {100 * r['observed']:.1f} % | {r['V']} | {r['F']} | "
                     + ", ".join(f"{x:.3f}" for x in r["integrate_ms"]) + " | " + ", ".join(f"{x:.3f}" for x in r["extract_ms"])
                     + f" | {r['identical_bytes']} |")
    lines += ["", "Kernel times (`rocprofv3 --kernel-trace --stats` around `--workload`, a run of its own, one per case):", "",
              "| case | kernel | calls | average (ms) | rate |", "|---|---|---|---|---|"]
    for r in rows:
        if not r["kernels"]:
            lines.append(f"| {r['case']} | all | - | not measured | - |")
            continue
        ext_ns = 0.0
        for name, (calls, ns) in sorted(r["kernels"].items()):
            rate = "-"
            if name == "k_tsdf_voxels":
                rate = (f"{r['pairs'] / (ns * 1e-9):.3g} pairs/s (`k_cons_count`: {YARDSTICK[0] / YARDSTICK[1]:.3g} pairs/s, the same "
                        "per-pair work on candidates only: a yardstick)")
            if name in ("k_tsdf_cells", "k_tsdf_count_edges", "k_tsdf_vertices", "k_tsdf_faces", "k_scan_counts"):
                ext_ns += ns
            lines.append(f"| {r['case']} | `{name}` | {calls} | {ns * 1e-6:.4f} | {rate} |")
        if ext_ns:
            share = r["extract_bytes"] / (ext_ns * 1e-9) / HBM_PEAK
            lines.append(f"| {r['case']} | extraction, five kernels | - | {ext_ns * 1e-6:.4f} | {r['extract_bytes']:.3g} algorithmic bytes: "
                         f"{100 * share:.1f} % of the 8 TB/s HBM peak |")
    lines += ["", "Registers, LDS and scratch of every kernel are in DESIGN.md section 7i (from the compiler's resource report).  "
              "No frustum cull is implemented, so there is nothing to alternate against.", "", "```json", json.dumps(rows), "```", ""]
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
