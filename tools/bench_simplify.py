"""Device time of the mesh simplification: simplify.simplify_mesh on the two meshes the project produces.

    python tools/bench_simplify.py [--out profiles/simplify_bench.md] [--cases fused,keyframes] [--factors 2,4,8]
                                   [--stats fused:8=DIR,keyframes:2=DIR,...]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_simplify.py --workload --cases fused --factors 8

fused: the default fused mesh of the 256:16 case of tools/bench_tsdf.py (a cube of 256^3 voxels over 16 keyframes of
512 x 512 that see one surface), beside fusion.extract_surface on the same volume.  keyframes: export.collect_mesh of 8
keyframes of 512 x 512 at stride 1, beside collect_mesh itself.  The voxel is a factor times the mesh's own spacing, the
median length of the first edge of its faces: a surface has about factor^2 vertices per cluster, so 8 is the coarse case.

Call times: a host clock around calls that end in a device synchronise, median of 5 rounds after a warm-up - the whole
simplify_mesh call (with its allocations and its one host read of the header) and the producer's call (with its own host
read) - and device events around eager calls of the two entry points on a prebuilt workspace and prebuilt outputs, where
nothing is read back.  Kernel times come from separate runs of `--workload` (the same calls, untimed, one case and one
factor each) under rocprofv3, whose output directories are given with --stats; without them the kernel table says "not
measured".

What a call has to move, from the shapes alone (SV, SF: the table slots, the power of two >= 2 V, 2 F):
  clear      64 SV + 4 SF written
  insert     15 V read, 8 V written, and the 64 bytes of a slot touched by each vertex's eight atomics
  leaders    12 V read, 4 V written
  faces      12 F read, three leaders (12 F) gathered, a table word and fslot (8 F)
  winners    8 F read
  scatter    4 V + 8 F read; per output vertex its slot (64) and 19 written; per output face 24 read, 20 written
That sum is shown beside the time a device-to-device copy of as many bytes takes on the same box (measured here with a
256 MiB copy).  The probes of the two tables and the rebuilt keys of occupied face slots add data-dependent loads that
this count leaves out."""
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
from mast3r_slam import _ffi, export, fusion, render, simplify  # noqa: E402

H = W = 512
ORIGIN, SIDE, D, K_FUSED, K_MESH = (-2.0, -2.0, 0.5), 4.0, 256, 16, 8
# The first version had every vertex do its own eight atomics; the same tool measured it before adjacent lanes with the same
# cell were merged inside the wave: (case, factor) -> (count stage device ms, median; k_sv_insert average ms or None).
PER_VERTEX_ATOMICS = {("fused", 2.0): (0.0560, 0.0351), ("fused", 4.0): (0.0573, None), ("fused", 8.0): (0.0693, 0.0546),
                      ("keyframes", 2.0): (0.3243, 0.2751), ("keyframes", 4.0): (0.3317, None), ("keyframes", 8.0): (0.3753, 0.3252)}
KERNELS = ("k_fill3", "k_sv_insert", "k_sv_leaders", "k_sv_faces", "k_sv_count_faces", "k_scan_counts", "k_sv_vertices",
           "k_sv_scatter_faces")


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
    """{kernel name: (calls, average ns)} of the simplify kernels in a rocprofv3 --stats directory.  k_scan_counts also runs
    in the producer: its row holds both."""
    hits = sorted(glob.glob(os.path.join(dirname, "**", "*kernel_stats.csv"), recursive=True))
    if not hits:
        raise SystemExit(f"no *kernel_stats.csv under {dirname}")
    out = {}
    for r in csv.DictReader(open(hits[0])):
        for key in KERNELS:
            if key + "(" in r["Name"] or r["Name"].endswith(key) or key + "E" in r["Name"]:
                out[key] = (int(r["Calls"]), float(r["AverageNs"]))
    return out


def copy_tb_per_s(dev):
    """Bytes read plus bytes written per second of a 256 MiB device-to-device copy, in TB/s."""
    src = torch.empty(1 << 28, dtype=torch.uint8, device=dev).fill_(1)
    dst = torch.empty_like(src)
    ms = event_ms(lambda: dst.copy_(src), 10)[0]
    return 2 * src.numel() / (ms * 1e-3) / 1e12


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


def slots(n):
    s = 1024
    while s < 2 * n:
        s *= 2
    return s


def bytes_moved(V, F, V2, F2):
    SV, SF = slots(V), slots(F)
    return (64 * SV + 4 * SF) + (15 + 8 + 64) * V + 16 * V + 32 * F + 8 * F + 4 * V + 8 * F + (64 + 19) * V2 + 44 * F2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_bench.md"))
    ap.add_argument("--cases", default="fused,keyframes")
    ap.add_argument("--factors", default="2,4,8")
    ap.add_argument("--stats", default="")
    ap.add_argument("--workload", action="store_true", help="run the calls untimed (for a profiler) and write nothing")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: nothing is measured without one")
    dev = torch.device("cuda:0")
    stats = dict(kv.split("=") for kv in a.stats.split(",") if kv)
    factors = [float(x) for x in a.factors.split(",")]
    L = _ffi.lib()
    copy_rate = None if a.workload else copy_tb_per_s(dev)
    rows = []
    for case in a.cases.split(","):
        make, name, hold = producer(case, dev)
        v, c, f = make()[:3]
        V, F = int(v.shape[0]), int(f.shape[0])
        fl = f.long()
        spacing = float((v[fl[:, 1]] - v[fl[:, 0]]).norm(dim=1).median())
        del fl
        ws = torch.empty(simplify.workspace_bytes(V, F), dtype=torch.uint8, device=dev)
        reps = max(4, min(100, (1 << 24) // max(F, 1)))
        producer_ms = None if a.workload else host_ms(make, reps)
        for factor in factors:
            voxel = float(np.float32(factor * spacing))
            call = lambda: simplify.simplify_mesh(v, c, f, voxel_size=voxel)
            out = call()
            torch.cuda.synchronize()
            if a.workload:
                for _ in range(3):
                    make()
                    call()
                torch.cuda.synchronize()
                continue
            again = call()
            same = all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(out, again))
            info = simplify.simplify_counts(v, c, f, voxel_size=voxel)
            V2, F2 = int(out[0].shape[0]), int(out[2].shape[0])
            st = _ffi.stream_ptr()
            count = lambda: _ffi.call("m3_mesh_simplify_count", _ffi.ptr(v), _ffi.ptr(c), _ffi.ptr(f), V, F, voxel, _ffi.ptr(ws),
                                      ws.numel(), st)
            scatter = lambda: _ffi.call("m3_mesh_simplify_scatter", _ffi.ptr(v), _ffi.ptr(c), _ffi.ptr(f), V, F, _ffi.ptr(ws),
                                        ws.numel(), V2, F2, _ffi.ptr(out[0]), _ffi.ptr(out[1]), _ffi.ptr(out[2]), None, None, st)
            count(), scatter()
            torch.cuda.synchronize()
            assert ws[:8].view(torch.int32).tolist() == [V2, F2]
            moved = bytes_moved(V, F, V2, F2)
            row = dict(case=case, producer=name, factor=factor, voxel=voxel, spacing=spacing, V=V, F=F, V2=V2, F2=F2,
                       out_of_range=info.out_of_range, per_cluster=V / max(V2, 1), identical_bytes=bool(same),
                       launches=int(L.m3_mesh_simplify_launches()), ws_bytes=int(ws.numel()), producer_ms=producer_ms,
                       call_ms=host_ms(call, reps), count_ms=event_ms(count, reps), scatter_ms=event_ms(scatter, reps),
                       bytes_moved=moved, copy_tb_per_s=copy_rate, copy_ms=moved / (copy_rate * 1e12) * 1e3)
            key = f"{case}:{a.factors.split(',')[factors.index(factor)]}"
            row["kernels"] = kernel_stats(stats[key]) if key in stats else None
            rows.append(row)
            print(json.dumps(row), flush=True)
            del out, again
        del hold, make, v, c, f, ws
        torch.cuda.empty_cache()
    if a.workload:
        return
    t3 = lambda x: ", ".join(f"{y:.3f}" for y in x)
    lines = ["# Mesh simplification: `simplify.simplify_mesh`", "",
             "Tool: `python tools/bench_simplify.py` (its docstring says what is timed and how the bytes are counted).  "
             f"Device: {torch.cuda.get_device_name(0)}.  Nothing here is a gate.", "",
             f"Launches per call: {rows[0]['launches'] if rows else 8} (6 to count, 2 to scatter), whatever the mesh holds.  Times in ms: "
             f"median, min, max of 5 rounds.  Device-to-device copy on this box: {copy_rate:.2f} TB/s (read plus written).", "",
             "| case | voxel / spacing | V -> V2 | F -> F2 | vertices per cluster | producer | producer call with its host read | "
             "`simplify_mesh` call with its host read | count, device | scatter, device | bytes moved | a copy of as many bytes | "
             "workspace bytes | identical bytes |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['factor']:g} | {r['V']} -> {r['V2']} | {r['F']} -> {r['F2']} | {r['per_cluster']:.1f} | "
                     f"`{r['producer']}` | {t3(r['producer_ms'])} | {t3(r['call_ms'])} | {t3(r['count_ms'])} | {t3(r['scatter_ms'])} | "
                     f"{r['bytes_moved']} | {r['copy_ms']:.3f} | {r['ws_bytes']} | {r['identical_bytes']} |")
    lines += ["", "Kernel times (`rocprofv3 --kernel-trace --stats` around `--workload`, a run of its own per row; `k_scan_counts` is "
              "also launched by the producer, so its row averages both):", "",
              "| case | voxel / spacing | kernel | calls | average (ms) |", "|---|---|---|---|---|"]
    for r in rows:
        if not r["kernels"]:
            lines.append(f"| {r['case']} | {r['factor']:g} | all | - | not measured |")
            continue
        for kname in KERNELS:
            if kname in r["kernels"]:
                calls, ns = r["kernels"][kname]
                lines.append(f"| {r['case']} | {r['factor']:g} | `{kname}` | {calls} | {ns * 1e-6:.4f} |")
    lines.append("")
    for r in rows:
        dev_ms = r["count_ms"][0] + r["scatter_ms"][0]
        text = (f"* {r['case']} at {r['factor']:g} spacings: the call takes {r['call_ms'][0]:.3f} ms ({dev_ms:.3f} ms on the device) beside "
                f"{r['producer_ms'][0]:.3f} ms for `{r['producer']}` and {r['copy_ms']:.3f} ms for a copy of the bytes it moves.")
        own = {k: ns for k, (_, ns) in (r["kernels"] or {}).items() if k.startswith("k_sv_")}
        if own:
            top = max(own, key=own.get)
            text += (f"  Of its own kernels `{top}` takes the most: {own[top] * 1e-6:.3f} of {sum(own.values()) * 1e-6:.3f} ms "
                     f"({100 * own[top] / sum(own.values()):.0f} %).")
        lines.append(text)
    lines += ["", "## What was measured and tried", "",
              "The first version had one thread per vertex do its own eight atomics (claim, leader row, count, three offset sums, "
              "three colour sums).  Its kernel `k_sv_insert` took 85 to 90 % of the count stage on the keyframe mesh, where "
              "neighbouring lanes share a cell and the adds pile onto few addresses.  The shipped kernel adds up each run of adjacent "
              "lanes with the same cell inside the wave (a segmented shuffle sum of five 32-bit words) and lets the run's first lane "
              "probe, claim and add once.  The sums are integers, so the bytes are the same.  Per-vertex atomics as this tool "
              "measured them before the change, merged runs from this run:", "",
              "| case | voxel / spacing | count stage, per-vertex atomics (ms) | merged runs (ms) | `k_sv_insert`, per-vertex atomics (ms) | "
              "merged runs (ms) |", "|---|---|---|---|---|---|"]
    for r in rows:
        old = PER_VERTEX_ATOMICS.get((r["case"], r["factor"]))
        if old:
            ins = (r["kernels"] or {}).get("k_sv_insert")
            lines.append(f"| {r['case']} | {r['factor']:g} | {old[0]:.4f} | {r['count_ms'][0]:.4f} | " +
                         (f"{old[1]:.4f}" if old[1] else "-") + " | " + (f"{ins[1] * 1e-6:.4f}" if ins else "-") + " |")
    lines += ["", "The merge helps most at a coarse voxel, where the runs are long.  At a fine voxel a cell is still shared by the "
              "pixel rows above and below and by the other keyframes, which are other waves: `k_sv_insert` stays the largest kernel "
              "there.  Not tried: merging through LDS across the waves of a workgroup, sorting the vertices by cell first, packing "
              "two sums into one word (the exact 2^55 and 2^39 ranges leave no room), and a clear that skips the sums of empty slots "
              "(the clear writes 64 bytes per slot of a table that is at most half full)."]
    lines += ["", "```json", json.dumps(rows), "```", ""]
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
