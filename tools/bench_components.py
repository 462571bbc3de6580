"""Device time of the mesh clean-up: components.filter_components on the two meshes the project produces.

    python tools/bench_components.py [--out profiles/components_bench.md] [--cases fused,keyframes] [--stats fused=DIR,keyframes=DIR]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_components.py --workload --cases fused

fused: the default fused mesh of the 256:16 case of tools/bench_tsdf.py (a cube of 256^3 voxels over 16 keyframes of
512 x 512 that see one surface, threshold 1.5), beside fusion.extract_surface on the same volume.  keyframes:
export.collect_mesh of 8 keyframes of 512 x 512 at stride 1, beside collect_mesh itself.  The filter is min_faces = 100.

Call times: a host clock around calls that end in a device synchronise, median of 5 rounds after a warm-up - the whole
filter_components call (with its allocations and its one host read of the header) and the producer's call (with its own
host read) - and device events around eager calls of each entry point on a prebuilt workspace and prebuilt outputs, where
nothing is read back.  Kernel times come from a separate run of `--workload` (the same calls, untimed) under rocprofv3,
whose output directory is given with --stats; without it the kernel table says "not measured".

What the kernels have to move, from the shapes alone: label reads the faces twice (12 F bytes each) and writes or reads
the four int32 arrays of V rows about eight times; count reads label and count per vertex and the faces once; scatter
reads the faces and the vertex arrays and writes 15 + 4 bytes per kept vertex and 12 per kept face.  The union-find walks
add data-dependent loads that this count leaves out."""
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
from mast3r_slam import _ffi, components, export, fusion, render  # noqa: E402

H = W = 512
ORIGIN, SIDE, D, K_FUSED, K_MESH = (-2.0, -2.0, 0.5), 4.0, 256, 16, 8
MIN_FACES = 100
TSDF_BENCH_EXTRACT_MS = 0.247                  # profiles/tsdf_bench.md, case 256:16: extract_surface with its host read, median
KERNELS = ("k_cc_init", "k_cc_hook", "k_cc_flatten", "k_cc_count_faces", "k_cc_winner", "k_cc_finish", "k_cc_count_vertices",
           "k_cc_count_kept_faces", "k_scan_counts", "k_cc_vertices", "k_cc_faces")


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
    """{kernel name: (calls, average ns)} of the component kernels in a rocprofv3 --stats directory.  k_scan_counts also
    runs in the producer: its row holds both."""
    hits = sorted(glob.glob(os.path.join(dirname, "**", "*kernel_stats.csv"), recursive=True))
    if not hits:
        raise SystemExit(f"no *kernel_stats.csv under {dirname}")
    out = {}
    for r in csv.DictReader(open(hits[0])):
        for key in KERNELS:
            if key + "(" in r["Name"] or r["Name"].endswith(key) or key + "E" in r["Name"]:
                out[key] = (int(r["Calls"]), float(r["AverageNs"]))
    return out


def producer(case, dev):
    """(the call that makes the mesh, its name)."""
    if case == "fused":
        sc = CT.shared_scene(K_FUSED, H, W, seed=K_FUSED)
        frames = RS.frames_of(sc, dev)
        volume = fusion.fuse_tsdf(render.map_tables(frames), CT.shared_pinhole(H, W), SIDE / D,
                                  out=fusion.empty_volume(ORIGIN, (D, D, D), SIDE / D, device=dev))
        return (lambda: fusion.extract_surface(volume)), "extract_surface", frames
    if case == "keyframes":
        sc = CT.shared_scene(K_MESH, H, W, seed=K_MESH)
        frames = RS.frames_of(sc, dev)
        return (lambda: export.collect_mesh(frames)), "collect_mesh", frames
    raise SystemExit(f"unknown case {case!r}: fused or keyframes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_bench.md"))
    ap.add_argument("--cases", default="fused,keyframes")
    ap.add_argument("--stats", default="")
    ap.add_argument("--workload", action="store_true", help="run the calls untimed (for a profiler) and write nothing")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: nothing is measured without one")
    dev = torch.device("cuda:0")
    stats = dict(kv.split("=") for kv in a.stats.split(",") if kv)
    L = _ffi.lib()
    rows = []
    for case in a.cases.split(","):
        make, name, hold = producer(case, dev)
        v, c, f = make()[:3]
        V, F = int(v.shape[0]), int(f.shape[0])
        clean = lambda: components.filter_components(v, c, f, min_faces=MIN_FACES)
        out = clean()
        torch.cuda.synchronize()
        if a.workload:
            for _ in range(3):
                make()
                clean()
            torch.cuda.synchronize()
            continue
        info = components.mesh_components(f, V)[2]
        again = clean()
        same = all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(out, again))
        ws = torch.empty(components.workspace_bytes(V, F), dtype=torch.uint8, device=dev)
        V2, F2 = int(out[0].shape[0]), int(out[2].shape[0])
        st = _ffi.stream_ptr()
        label = lambda: _ffi.call("m3_mesh_components_label", _ffi.ptr(f), V, F, _ffi.ptr(ws), ws.numel(), None, None, st)
        count = lambda: _ffi.call("m3_mesh_components_count", _ffi.ptr(ws), V, F, _ffi.ptr(f), MIN_FACES, 0.0, 0, st)
        scatter = lambda: _ffi.call("m3_mesh_components_scatter", _ffi.ptr(v), _ffi.ptr(c), _ffi.ptr(f), V, F, _ffi.ptr(ws), V2, F2,
                                    _ffi.ptr(out[0]), _ffi.ptr(out[1]), _ffi.ptr(out[2]), None, None, st)
        label(), count(), scatter()
        torch.cuda.synchronize()
        assert ws[:8].view(torch.int32).tolist() == [V2, F2]
        reps = max(4, min(200, (1 << 25) // max(F, 1)))
        row = dict(case=case, producer=name, V=V, F=F, V2=V2, F2=F2, components=info.components, largest=info.largest,
                   identical_bytes=bool(same), launches=int(L.m3_mesh_components_launches()), ws_bytes=int(ws.numel()),
                   producer_ms=host_ms(make, reps), clean_ms=host_ms(clean, reps), label_ms=event_ms(label, reps),
                   count_ms=event_ms(count, reps), scatter_ms=event_ms(scatter, reps))
        row["kernels"] = kernel_stats(stats[case]) if case in stats else None
        rows.append(row)
        print(json.dumps(row), flush=True)
        del hold, make, v, c, f, out, again, ws
        torch.cuda.empty_cache()
    if a.workload:
        return
    t3 = lambda x: ", ".join(f"{y:.3f}" for y in x)
    lines = ["# Mesh clean-up: `components.filter_components`", "",
             "Tool: `python tools/bench_components.py` (its docstring says what is timed).  "
             f"Device: {torch.cuda.get_device_name(0)}.  Nothing here is a gate, and nothing was tuned.", "",
             f"Filter: `min_faces = {MIN_FACES}`.  Launches per call: {rows[0]['launches'] if rows else 11} (6 to label, 3 to count, 2 to "
             "scatter), whatever the mesh holds.  Times in ms: median, min, max of 5 rounds.", "",
             "| case | V | F | components | largest | kept V2 | kept F2 | producer | producer call with its host read | "
             "`filter_components` call with its host read | label, device | count, device | scatter, device | identical bytes |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['V']} | {r['F']} | {r['components']} | {r['largest']} | {r['V2']} | {r['F2']} | `{r['producer']}` | "
                     f"{t3(r['producer_ms'])} | {t3(r['clean_ms'])} | {t3(r['label_ms'])} | {t3(r['count_ms'])} | {t3(r['scatter_ms'])} | "
                     f"{r['identical_bytes']} |")
    lines += ["", "Kernel times (`rocprofv3 --kernel-trace --stats` around `--workload`, a run of its own, one per case; "
              "`k_scan_counts` is also launched by the producer, so its row averages both):", "",
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
        ratio = r["clean_ms"][0] / r["producer_ms"][0]
        text = (f"* {r['case']}: the clean-up call takes {r['clean_ms'][0]:.3f} ms, `{r['producer']}` {r['producer_ms'][0]:.3f} ms on the same "
                f"input: {ratio:.1f} x" + (" - the clean-up costs more than the step it follows" if ratio > 1 else "") + ".")
        if r["case"] == "fused":
            text += f"  `profiles/tsdf_bench.md` has {TSDF_BENCH_EXTRACT_MS} ms for this extraction."
        own = {k: ns for k, (_, ns) in (r["kernels"] or {}).items() if k.startswith("k_cc_")}
        if own:
            top = max(own, key=own.get)
            text += (f"  Of its own kernels `{top}` dominates: {own[top] * 1e-6:.3f} of {sum(own.values()) * 1e-6:.3f} ms "
                     f"({100 * own[top] / sum(own.values()):.0f} %).")
        lines.append(text)
    lines += ["", "Not tuned: the figures are those of the first working version.", "", "```json", json.dumps(rows), "```", ""]
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
