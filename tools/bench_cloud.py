"""Device time of the point-cloud neighbourhoods: cloud.cloud_neighbors, cloud.cloud_normals and
cloud.remove_radius_outliers on a cloud of the production size.

    python tools/bench_cloud.py [--out profiles/cloud_bench.md] [--voxel 0.01] [--factors 2,3,4] [--stats 3=DIR,...]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_cloud.py --workload --factors 3

The cloud is export.collect_map of the keyframes of tools/bench_simplify.py (8 keyframes of 512 x 512 that see one
surface), thinned to one point per voxel; the radius is 2, 3 and 4 voxel edges.

Times: device events around eager calls of the entry points on a prebuilt workspace - m3_cloud_neighbors with and
without the moments (7 launches each) and m3_cloud_normals (1 launch) - and a host clock around the whole Python calls,
which end in a device synchronise (cloud_normals with its one 16-byte read; remove_radius_outliers with its read and
its scatter); median, min and max of 5 rounds after a warm-up.  Kernel times come from separate runs of `--workload`
under rocprofv3, whose output directories are given with --stats; without them the kernel table says "not measured".

Pairs.  A query visits every point of the 27 cells around its own: the candidates.  Their number is counted here with
torch (cells, unique keys, 27 look-ups), independently of the kernels; the neighbours are the sum of `count`.  Each
candidate is one 16-byte load, nearly all of them served by the caches, since the lanes of a wave walk the same few
cells.  What the pass has to move through HBM once, from the shapes alone (S table slots):
  12 M read (points, twice: insert and fill), 8 M (slot, rank: written and read), 20 M written and 20 M read (the
  cell-sorted list and its slots), 8 S + 4 S cleared, 8 S + 4 S read (keys and cell starts), 4 M + 72 M written
  (count, moments)
It is shown as the time a device-to-device copy of as many bytes takes on the same box (measured with a 256 MiB copy):
the floor no ordering of the cells can get under.  The LDS-staged variant of the walk (the lanes of a workgroup share
the ranges of their cells through LDS) was not built, so there is no second column for it."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mast3r-slam_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import bench_simplify as BS  # noqa: E402  (the keyframes, the timers and the copy rate)
from mast3r_slam import _ffi, cloud, export  # noqa: E402

# A variant of the moment sums as this tool timed it against the shipped one (profiles/cloud_bench.md says what A and B
# were): radius / voxel -> neighbour pass with moments, device ms, median of the two runs of (A, B).
TRIED = {"2": (0.2981, 0.3755), "3": (0.5530, 0.6563), "4": (0.8917, 1.0061)}
KERNELS = ("k_fill2", "k_cl_insert", "k_tile_sums", "k_scan_counts", "k_row_starts", "k_cl_fill", "k_cl_query",
           "k_cl_normals", "k_cl_keep_count", "k_cl_keep_scatter")


def candidates(points, radius):
    """Points in the 27 cells around every finite point, added up: what the walk visits."""
    r = float(np.float32(radius))
    h = r * (1.0 + 2.0 ** -10)
    p = points[torch.isfinite(points).all(dim=1)].double()
    c = torch.floor(p / h).long() + (1 << 20)
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    uniq, inverse, per_cell = torch.unique(key, return_inverse=True, return_counts=True)
    total = 0
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                want = uniq + ((dx << 42) + (dy << 21) + dz)
                at = torch.searchsorted(uniq, want).clamp_(max=uniq.numel() - 1)
                hit = uniq[at] == want
                total += int((per_cell * torch.where(hit, per_cell[at], torch.zeros_like(per_cell))).sum())
    return total, int(uniq.numel()), int(per_cell.max())


def slots(m):
    s = 1024
    while s < 2 * m:
        s *= 2
    return s


def kernel_stats(dirname):
    """{kernel: (calls, average ns)} of a rocprofv3 --stats directory; the two instances of k_cl_query are added up, and
    k_scan_counts also runs in the producer."""
    import csv
    import glob
    hits = sorted(glob.glob(os.path.join(dirname, "**", "*kernel_stats.csv"), recursive=True))
    if not hits:
        raise SystemExit(f"no *kernel_stats.csv under {dirname}")
    tot = {}
    for r in csv.DictReader(open(hits[0])):
        for key in KERNELS:
            if key in r["Name"]:
                calls, ns = tot.get(key, (0, 0.0))
                tot[key] = (calls + int(r["Calls"]), ns + int(r["Calls"]) * float(r["AverageNs"]))
    return {k: (calls, ns / calls) for k, (calls, ns) in tot.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_bench.md"))
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--factors", default="2,3,4")
    ap.add_argument("--stats", default="")
    ap.add_argument("--workload", action="store_true", help="run the calls untimed (for a profiler) and write nothing")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: nothing is measured without one")
    dev = torch.device("cuda:0")
    stats = dict(kv.split("=") for kv in a.stats.split(",") if kv)
    L = _ffi.lib()
    _, _, frames = BS.producer("keyframes", dev)
    pts = export.collect_map(frames, voxel_size=a.voxel, return_index=True)
    toward = cloud.source_viewpoints(frames, pts[2])
    p = pts[0]
    M = int(p.shape[0])
    copy_rate = None if a.workload else BS.copy_tb_per_s(dev)
    rows = []
    for factor in a.factors.split(","):
        radius = float(np.float32(float(factor) * a.voxel))
        normals = lambda: cloud.cloud_normals(p, radius, toward=toward)
        keep = lambda: cloud.remove_radius_outliers(pts, radius=radius, min_neighbors=4)
        first = normals()
        kept = keep()
        torch.cuda.synchronize()
        if a.workload:
            for _ in range(3):
                normals(), keep()
            torch.cuda.synchronize()
            continue
        same = first.cpu().numpy().tobytes() == normals().cpu().numpy().tobytes()
        nb = cloud.cloud_neighbors(p, radius)
        ws = torch.empty(cloud.workspace_bytes(M), dtype=torch.uint8, device=dev)
        out = torch.empty((M, 3), dtype=torch.float32, device=dev)
        st, scale = _ffi.stream_ptr(), 2.0 ** 20 / radius
        walk = lambda mom: _ffi.call("m3_cloud_neighbors", _ffi.ptr(p), M, radius, scale, _ffi.ptr(nb.count), _ffi.ptr(mom),
                                     _ffi.ptr(ws), ws.numel(), st)
        finish = lambda: _ffi.call("m3_cloud_normals", _ffi.ptr(p), M, _ffi.ptr(nb.count), _ffi.ptr(nb.moments), _ffi.ptr(toward), 3,
                                   3, _ffi.ptr(out), None, st)
        walk(nb.moments), walk(None), finish()
        torch.cuda.synchronize()
        visited, cells, longest = candidates(p, radius)
        pairs = int(nb.count.sum(dtype=torch.int64))
        S = slots(M)
        once = 12 * M + 8 * M + 40 * M + 24 * S + 76 * M
        reps = 100
        with_ms, without_ms = BS.event_ms(lambda: walk(nb.moments), reps), BS.event_ms(lambda: walk(None), reps)
        row = dict(factor=float(factor), voxel=a.voxel, radius=radius, M=M, cells=cells, longest_cell=longest,
                   mean_neighbours=pairs / max(M, 1), max_neighbours=int(nb.count.max()), candidates=visited, pairs=pairs,
                   neighbors_ms=with_ms, counts_only_ms=without_ms, normals_ms=BS.event_ms(finish, reps),
                   cloud_normals_call_ms=BS.host_ms(normals, reps), filter_call_ms=BS.host_ms(keep, reps), kept=int(kept[0].shape[0]),
                   candidates_per_s=visited / (with_ms[0] * 1e-3), pairs_per_s=pairs / (with_ms[0] * 1e-3),
                   candidate_bytes_tb_per_s=16 * visited / (with_ms[0] * 1e-3) / 1e12, launches=int(L.m3_cloud_launches()),
                   ws_bytes=int(ws.numel()), once_bytes=once, copy_tb_per_s=copy_rate, copy_ms=once / (copy_rate * 1e12) * 1e3,
                   identical_bytes=bool(same), kernels=kernel_stats(stats[factor]) if factor in stats else None)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del ws, out, nb
        torch.cuda.empty_cache()
    if a.workload:
        return
    t3 = lambda x: ", ".join(f"{y:.4f}" for y in x)
    lines = ["# Point-cloud neighbourhoods: `cloud.cloud_neighbors`, `cloud.cloud_normals`, `cloud.remove_radius_outliers`", "",
             "Tool: `python tools/bench_cloud.py` (its docstring says what is timed and how pairs and bytes are counted).  "
             f"Device: {torch.cuda.get_device_name(0)} (the library is built for gfx950 alone: an MI355X).  Nothing here is a gate: "
             "there is no earlier implementation to compare with, and these are the numbers a later change improves on.", "",
             f"Cloud: `collect_map` of 8 keyframes of 512 x 512 that see one surface, one point per voxel of {a.voxel}: {M} points.  "
             f"Launches: {rows[0]['launches'] if rows else 7} for the neighbour pass whatever the cloud holds, one for the normals, "
             "three for the filter.  Times in ms: median, min, max of 5 rounds.  Device-to-device copy on this box: "
             f"{copy_rate:.2f} TB/s (read plus written).  The LDS-staged walk was not built: one column.", "",
             "| radius / voxel | occupied cells | longest cell | mean neighbours | max | candidates visited | neighbour pass with moments, "
             "device | counts only, device | candidates per second | neighbour pairs per second | candidate bytes (16 each) | bytes moved "
             "once | a copy of as many bytes | normals pass, device | `cloud_normals`, whole call | `remove_radius_outliers`, whole call | "
             "workspace bytes | identical bytes |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['factor']:g} | {r['cells']} | {r['longest_cell']} | {r['mean_neighbours']:.1f} | {r['max_neighbours']} | "
                     f"{r['candidates']} | {t3(r['neighbors_ms'])} | {t3(r['counts_only_ms'])} | {r['candidates_per_s']:.3e} | "
                     f"{r['pairs_per_s']:.3e} | {r['candidate_bytes_tb_per_s']:.2f} TB/s | {r['once_bytes']} | {r['copy_ms']:.4f} | "
                     f"{t3(r['normals_ms'])} | {t3(r['cloud_normals_call_ms'])} | {t3(r['filter_call_ms'])} | {r['ws_bytes']} | "
                     f"{r['identical_bytes']} |")
    lines += ["", "Kernel times (`rocprofv3 --kernel-trace --stats` around `--workload`, a run of its own per radius; the two instances "
              "of `k_cl_query` are added up, and `k_scan_counts` is also launched by the producer):", "",
              "| radius / voxel | kernel | calls | average (ms) |", "|---|---|---|---|"]
    for r in rows:
        if not r["kernels"]:
            lines.append(f"| {r['factor']:g} | all | - | not measured |")
            continue
        for kname in KERNELS:
            if kname in r["kernels"]:
                calls, ns = r["kernels"][kname]
                lines.append(f"| {r['factor']:g} | `{kname}` | {calls} | {ns * 1e-6:.4f} |")
    lines.append("")
    for r in rows:
        lines.append(f"* radius {r['factor']:g} voxels: the neighbour pass takes {r['neighbors_ms'][0]:.3f} ms on the device, "
                     f"{r['neighbors_ms'][0] / r['copy_ms']:.1f} times a copy of the {r['once_bytes']} bytes it has to move once; it visits "
                     f"{r['candidates'] / max(r['pairs'], 1):.1f} candidates per neighbour found.")
    lines += ["", "## What was measured and tried", "",
              "The walk is bound by its arithmetic, not by memory: the same seven launches without the moments (three float64 "
              "subtractions, `d2` and a compare per candidate) take half to two thirds of the time of the pass with them, and the candidate "
              "loads - 16 bytes each, several TB/s in the table above - come from the caches, since the lanes that share a cell "
              "issue the same addresses.  That is why the LDS-staged walk was not built first: it removes loads, not arithmetic.  "
              "One variant of the arithmetic was built and timed against the shipped one, the two libraries alternating A B A B "
              "in one job on the same cloud, 100 calls per round (the spread between the two runs of a variant was below 0.3 %); "
              "`count` and `moments` were the twin's bytes for both.  A (shipped): the offsets quantised to int32, the nine sums "
              "in int64 by 32 x 32 + 64-bit multiply-adds (`v_mad_i64_i32`), 52 VGPR.  B: the sums kept exactly in float64 "
              "(`v_fma_f64` on integers below 2^52, moved to the int64 accumulators every 512 candidates), 114 VGPR.  "
              "Neighbour pass with moments, device, ms:", "",
              "| radius / voxel | A | B |", "|---|---|---|"]
    lines += [f"| {f} | {x:.4f} | {y:.4f} |" for f, (x, y) in TRIED.items()]
    lines += ["", "B is 13 to 26 % slower: it halves the waves a SIMD holds and saves nothing the integer path was short of.  Not "
              "tried: staging the cell ranges of a workgroup through LDS; laying the cells out along a space-filling curve, so "
              "that neighbouring cells are neighbours in memory (they lie in hash order now); a float32 pre-test of `d2` with a "
              "margin, leaving float64 to the candidates near the boundary; one wave per cell, the candidates held in registers "
              "and passed round by `v_readlane`."]
    lines += ["", "```json", json.dumps(rows), "```", ""]
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
