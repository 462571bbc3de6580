"""Device time of the mesh smoothing: smooth.smooth_mesh and smooth.mesh_topology on the two meshes the project produces.

    python tools/bench_smooth.py [--out profiles/smooth_bench.md] [--cases fused,keyframes,hub] [--stats fused=DIR,keyframes=DIR,...]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_smooth.py --workload --cases fused

fused and keyframes: the meshes of tools/bench_simplify.py (the fused surface of a 256^3 volume over 16 keyframes of
512 x 512; export.collect_mesh of 8 keyframes of 512 x 512).  hub: a synthetic fan, one vertex with 4096 neighbours, for
what the longest row costs - the rows of the two real meshes have about six entries.

Call times: a host clock around calls that end in a device synchronise, median of 5 rounds after a warm-up - the whole
smooth_mesh call with the defaults (10 Taubin iterations: 7 launches for the topology and 20 passes, nothing read back)
and the whole mesh_topology call (with its one host read) - and device events around eager calls of the entry points on
a prebuilt workspace: m3_mesh_topology_build alone, and m3_mesh_smooth_passes with 20 passes, divided by 20.  Kernel
times come from separate runs of `--workload` (the same calls, untimed, one case each) under rocprofv3, whose output
directories are given with --stats; without them the kernel table says "not measured".

What a pass between two position buffers has to move, from the shapes alone (E edges, so 2 E adjacency entries):
  once each  16 V read (the positions), 4 (V + 1) read (off), 8 E read (nbr), 16 V written
  gathered   32 E: one 16-byte load per adjacency entry, served by the caches when neighbours lie near each other
The first figure is what no ordering of the vertices can avoid; it is shown beside the time a device-to-device copy of
as many bytes takes on the same box (measured here with a 256 MiB copy)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mast3r-slam_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import bench_simplify as BS  # noqa: E402  (the two producers, the timers and the copy rate)
from mast3r_slam import _ffi, smooth  # noqa: E402

HUB = 4096
PASSES = 20
# Earlier versions of the build stage as this tool measured them (profiles/smooth_bench.md says what A and B were):
# case -> version -> (build stage device ms, median; scan kernels; k_sm_fill; k_sm_sort - rocprofv3 averages, ms).
EARLIER = {"fused": {"A": (0.1966, 0.0446, 0.0765, 0.0205), "B": (0.1596, 0.0199, 0.0769, 0.0217)},
           "keyframes": {"A": (1.3980, 0.3590, 0.7945, 0.0179), "B": (0.9650, 0.0155, 0.7757, 0.0182)},
           "hub": {"A": (10.9507, 0.0049, 0.0517, 10.8652), "B": (2.2886, 0.0139, 0.0500, 2.1741)}}
KERNELS = ("k_fill2", "k_sm_faces", "k_tile_sums", "k_scan_counts", "k_row_starts", "k_sm_fill", "k_sm_sort", "k_sm_read", "k_sm_pass", "k_sm_copy")


def hub_mesh(dev):
    """One hub (row 0) with HUB rim vertices around it."""
    t = torch.arange(HUB, dtype=torch.float32) * (2.0 * np.pi / HUB)
    v = torch.cat([torch.tensor([[0.0, 0.0, 0.3]]), torch.stack([t.cos(), t.sin(), torch.zeros(HUB)], dim=1)])
    i = torch.arange(HUB, dtype=torch.int32)
    f = torch.stack([torch.zeros(HUB, dtype=torch.int32), 1 + i, 1 + (i + 1) % HUB], dim=1)
    return v.to(dev), torch.zeros((HUB + 1, 3), dtype=torch.uint8, device=dev), f.to(dev)


def kernel_stats(dirname):
    """{kernel: (calls, average ns)} of a rocprofv3 --stats directory; the four k_sm_pass instances are added up, and
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_bench.md"))
    ap.add_argument("--cases", default="fused,keyframes,hub")
    ap.add_argument("--stats", default="")
    ap.add_argument("--workload", action="store_true", help="run the calls untimed (for a profiler) and write nothing")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: nothing is measured without one")
    dev = torch.device("cuda:0")
    stats = dict(kv.split("=") for kv in a.stats.split(",") if kv)
    L = _ffi.lib()
    copy_rate = None if a.workload else BS.copy_tb_per_s(dev)
    rows = []
    for case in a.cases.split(","):
        hold = None
        if case == "hub":
            v, c, f = hub_mesh(dev)
        else:
            make, _, hold = BS.producer(case, dev)
            v, c, f = make()[:3]
        V, F = int(v.shape[0]), int(f.shape[0])
        call = lambda: smooth.smooth_mesh(v, c, f)
        topo = lambda: smooth.mesh_topology(f, V)
        out = call()[0]
        info = topo()
        torch.cuda.synchronize()
        if a.workload:
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            continue
        same = out.cpu().numpy().tobytes() == call()[0].cpu().numpy().tobytes()
        ws = torch.empty(smooth.workspace_bytes(V, F), dtype=torch.uint8, device=dev)
        st = _ffi.stream_ptr()
        build = lambda: _ffi.call("m3_mesh_topology_build", _ffi.ptr(f), V, F, _ffi.ptr(ws), ws.numel(), st)
        passes = lambda: _ffi.call("m3_mesh_smooth_passes", _ffi.ptr(v), V, F, _ffi.ptr(ws), ws.numel(), None, 0, 1, PASSES // 2,
                                   0.5, -0.53, _ffi.ptr(out), st)
        build(), passes()
        torch.cuda.synchronize()
        E = info.edges
        reps = max(4, min(100, (1 << 24) // max(F, 1)))
        once = 16 * V + 4 * (V + 1) + 8 * E + 16 * V
        pass_ms = tuple(x / PASSES for x in BS.event_ms(passes, reps))
        row = dict(case=case, V=V, F=F, E=E, boundary_edges=info.boundary_edges, nonmanifold_edges=info.nonmanifold_edges,
                   longest_row=int(info.degree.max()), mean_row=2.0 * E / max(V, 1), identical_bytes=bool(same),
                   build_launches=int(L.m3_mesh_smooth_launches()), ws_bytes=int(ws.numel()), call_ms=BS.host_ms(call, reps),
                   topology_ms=BS.host_ms(topo, reps), build_ms=BS.event_ms(build, reps), pass_ms=pass_ms, pass_bytes=once,
                   gathered_bytes=32 * E, copy_tb_per_s=copy_rate, copy_ms=once / (copy_rate * 1e12) * 1e3,
                   kernels=kernel_stats(stats[case]) if case in stats else None)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del hold, v, c, f, ws, out, info
        torch.cuda.empty_cache()
    if a.workload:
        return
    t3 = lambda x: ", ".join(f"{y:.4f}" for y in x)
    lines = ["# Mesh smoothing: `smooth.smooth_mesh` and `smooth.mesh_topology`", "",
             "Tool: `python tools/bench_smooth.py` (its docstring says what is timed and how the bytes are counted).  "
             f"Device: {torch.cuda.get_device_name(0)} (the library is built for gfx950 alone: an MI355X).  Nothing here is a gate.", "",
             f"Launches: {rows[0]['build_launches'] if rows else 7} for the topology whatever the mesh holds, then one per pass.  Times in ms: "
             f"median, min, max of 5 rounds.  Device-to-device copy on this box: {copy_rate:.2f} TB/s (read plus written).", "",
             "| case | V | F | E | boundary edges | non-manifold edges | mean row | longest row | `smooth_mesh`, 10 Taubin iterations, whole call | "
             "`mesh_topology`, whole call with its host read | topology build, device | one pass, device | bytes a pass moves once | "
             "a copy of as many bytes | gathered bytes | workspace bytes | identical bytes |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['V']} | {r['F']} | {r['E']} | {r['boundary_edges']} | {r['nonmanifold_edges']} | {r['mean_row']:.2f} | "
                     f"{r['longest_row']} | {t3(r['call_ms'])} | {t3(r['topology_ms'])} | {t3(r['build_ms'])} | {t3(r['pass_ms'])} | "
                     f"{r['pass_bytes']} | {r['copy_ms']:.4f} | {r['gathered_bytes']} | {r['ws_bytes']} | {r['identical_bytes']} |")
    lines += ["", "Kernel times (`rocprofv3 --kernel-trace --stats` around `--workload`, a run of its own per case; the four instances of "
              "`k_sm_pass` are added up, and `k_scan_counts` is also launched by the producer, so its row averages both):", "",
              "| case | kernel | calls | average (ms) |", "|---|---|---|---|"]
    for r in rows:
        if not r["kernels"]:
            lines.append(f"| {r['case']} | all | - | not measured |")
            continue
        for kname in KERNELS:
            if kname in r["kernels"]:
                calls, ns = r["kernels"][kname]
                lines.append(f"| {r['case']} | `{kname}` | {calls} | {ns * 1e-6:.4f} |")
    lines.append("")
    for r in rows:
        lines.append(f"* {r['case']}: the topology takes {r['build_ms'][0]:.3f} ms and a pass {r['pass_ms'][0]:.4f} ms on the device, "
                     f"{r['pass_ms'][0] / r['copy_ms']:.1f} times a copy of the {r['pass_bytes']} bytes it has to move once; the longest "
                     f"row has {r['longest_row']} entries.")
    lines += ["", "## What was measured and tried", "",
              "The build stage went through three versions, each measured with this tool on the same kind of box; the bytes never "
              "changed.  A: five launches - one single-workgroup `launch_scan` over all V + 1 degrees, the fill one thread per table "
              "slot with a cursor array and atomic ors for the boundary flags, long rows sorted by a wave whose lanes each read the "
              "whole row.  B: the scan in three launches (sums per tile, a scan of the tiles, tile offset + rank), the cursor "
              "folded into the row starts, the boundary flag carried in bit 31 of the row entries, the wave sort with 64 entries "
              "against 64 entries in registers.  C (shipped): B with the fill one thread per face, over the corners that claimed a "
              "slot.  Build stage on the device and kernel averages, ms:", "",
              "| case | build A | build B | build C (this run) | scan A | scan B (three kernels) | fill A | fill B | fill C (this run) | "
              "sort A | sort B | sort C (this run) |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        old = EARLIER.get(r["case"])
        if old:
            k = r["kernels"] or {}
            now = lambda name: f"{k[name][1] * 1e-6:.4f}" if name in k else "not measured"
            lines.append(f"| {r['case']} | {old['A'][0]:.4f} | {old['B'][0]:.4f} | {r['build_ms'][0]:.4f} | {old['A'][1]:.4f} | {old['B'][1]:.4f} | "
                         f"{old['A'][2]:.4f} | {old['B'][2]:.4f} | {now('k_sm_fill')} | {old['A'][3]:.4f} | {old['B'][3]:.4f} | {now('k_sm_sort')} |")
    lines += ["", "The single-workgroup scan took a quarter of build A on the keyframe mesh (751 147 degrees in 184 rounds of one "
              "workgroup; its row also averages the producer's own small scans); in three launches it is 0.015 ms.  Folding the "
              "cursor into the row starts and dropping the atomic ors did not move the fill (A to B): it is bound by its returning "
              "`atomicAdd`s, and from hash-ordered slots each of them, and each row write, goes to a cache line of its own.  The "
              "same adds issued in face order (C) land on the lines of neighbouring vertices.  The hub shows what a long row costs: "
              f"the sort of one row of {HUB} entries is nearly all of its build (a rank sort is quadratic in the row; B and C hold "
              "64 x 64 entries in registers per round where A read the row from memory for every entry), and a pass walks the "
              "row in its one thread, four loads at a time - the pass time of the hub case is that one thread.  Rows of the two "
              "real meshes have 6 to 18 entries.  Not tried: a wave per long row in the pass (the sum must stay in ascending order, "
              "so only the loads could be shared), a merge sort for rows of many thousands, vertex reordering for locality of the "
              "gather, and packing the positions as three 21-bit integers to halve the gathered bytes (it would change the rule)."]
    lines += ["", "```json", json.dumps(rows), "```", ""]
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
