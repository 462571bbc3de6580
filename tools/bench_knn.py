"""Device time of the k-nearest-neighbour query: cloud.cloud_knn beside the counts-only neighbour pass of the same library,
on the cloud of tools/bench_cloud.py.

    python tools/bench_knn.py [--out profiles/knn_bench.md] [--voxel 0.01] [--factor 3] [--ks 8,16,32]
                              [--variant-lib PATH] [--stats 8=DIR,16=DIR,...]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_knn.py --workload --ks 8

The cloud is export.collect_map of the keyframes of tools/bench_simplify.py (8 keyframes of 512 x 512 that see one
surface), thinned to one point per voxel; the radius is 3 voxel edges.

Times: device events around eager calls of the entry points on a prebuilt workspace, 100 calls per round, median, min
and max of 5 rounds after a warm-up.  m3_knn_query and the counts-only m3_cloud_neighbors both queue seven launches, and
the first six - the index build - are the same code on the same cloud.  Both query kernels visit the same candidates in
the same order, so the difference of the two calls is the price of the selection: the key, the compare, the LDS list,
the final sort and the [Q,k] outputs.  The kernels' own times come from separate runs of `--workload` under rocprofv3
(--stats); without them the kernel columns say "not measured".  Cross mode is timed with the points themselves as
queries, in shuffled order: the same candidates, but the lanes of a wave no longer share a cell.

Registers, scratch and LDS come from the metadata of the gfx950 code object inside the library (llvm-objdump
--offloading, llvm-readelf --notes); the list in LDS is dynamic, 8 k threads bytes per workgroup, so the static size is 0.

--variant-lib: another build of the library (M3SLAM_LIB), timed against the shipped one in fresh child processes that
alternate A B A B in this one job; each child reports its times and a SHA-256 of index, dist2 and found per k.  The
variant this file was written for is a copy of csrc/cloud.hip with the insertion written the other way, linked with the
shipped objects: the list kept in ascending order (a candidate that enters shifts the larger keys up, no final sort)
against the shipped one (unordered, the worst key and its position in registers, one scan of k words per entry, one
sort at the end).  The variant's source is not kept: profiles/knn_bench.md has what it was and what it measured."""
import argparse
import glob
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mast3r-slam_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import bench_simplify as BS  # noqa: E402  (the keyframes and the timers)
from mast3r_slam import _ffi, cloud, export  # noqa: E402

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
REPS = 100


def resources(lib_path):
    """{kernel: dict(threads, vgpr, sgpr, scratch, lds)} of the k_knn_* and k_cl_query kernels of the library's code object."""
    tmp = tempfile.mkdtemp(prefix="knn_co_")
    try:
        lib = shutil.copy(lib_path, tmp)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", lib], check=True, capture_output=True, cwd=tmp)
        out = {}
        for co in glob.glob(os.path.join(tmp, "*gfx950*")):
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            for block in notes.split("  - .agpr_count")[1:]:
                get = lambda key: re.search(r"^\s{4}\.%s:\s+(\S+)" % key, block, re.M).group(1)
                name = get("name")
                m = re.search(r"(k_knn_query|k_knn_moments|k_knn_mean_distance|k_cl_query)(ILi(\d+)ELb([01])E|ILb([01])E)?", name)
                if not m:
                    continue
                tag = m.group(1)
                if m.group(3):
                    tag += f"<{m.group(3)}, {'cross' if m.group(4) == '1' else 'self'}>"
                elif m.group(5):
                    tag += f"<{'moments' if m.group(5) == '1' else 'counts'}>"
                out[tag] = dict(threads=int(get("max_flat_workgroup_size")), vgpr=int(get("vgpr_count")), sgpr=int(get("sgpr_count")),
                                scratch=int(get("private_segment_fixed_size")), lds=int(get("group_segment_fixed_size")))
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def load_cloud(voxel, dev):
    _, _, frames = BS.producer("keyframes", dev)
    return export.collect_map(frames, voxel_size=voxel)[0]


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


def measure(p, radius, ks, cross, workload=False):
    """One row per k: device ms of the k-NN call, of the counts-only call, of the cross call; the completed fraction."""
    dev, M = p.device, int(p.shape[0])
    ws = torch.empty(cloud.workspace_bytes(M), dtype=torch.uint8, device=dev)
    st, scale = _ffi.stream_ptr(), 2.0 ** 20 / radius
    count = torch.empty((M,), dtype=torch.int32, device=dev)
    shuffled = p[torch.from_numpy(np.random.default_rng(0).permutation(M)).to(dev)].contiguous()
    counts = lambda: _ffi.call("m3_cloud_neighbors", _ffi.ptr(p), M, radius, scale, _ffi.ptr(count), None, _ffi.ptr(ws), ws.numel(), st)
    rows = []
    for k in ks:
        first = cloud.cloud_knn(p, k, radius)
        again = cloud.cloud_knn(p, k, radius, workspace=ws)
        index, dist2, found = again.index, again.dist2, again.found
        knn = lambda q=None: _ffi.call("m3_knn_query", _ffi.ptr(p), M, radius, _ffi.ptr(q), M, k, _ffi.ptr(index), _ffi.ptr(dist2),
                                       _ffi.ptr(found), _ffi.ptr(ws), ws.numel(), st)
        same = digest(first.index, first.dist2, first.found) == digest(index, dist2, found)
        sha = digest(index, dist2, found)
        complete = float((found == k).double().mean())
        counts(), knn(), torch.cuda.synchronize()
        if workload:
            for _ in range(10):
                counts(), knn()
            if cross:
                for _ in range(10):
                    knn(shuffled)
            torch.cuda.synchronize()
            continue
        row = dict(k=k, M=M, radius=radius, knn_ms=BS.event_ms(knn, REPS), counts_ms=BS.event_ms(counts, REPS),
                   knn_ms_again=BS.event_ms(knn, REPS), counts_ms_again=BS.event_ms(counts, REPS),
                   complete=complete, identical_bytes=bool(same), sha256=sha, threads=256 if k <= 16 else 128 if k <= 32 else 64,
                   launches=int(_ffi.lib().m3_knn_launches()))
        row["lds_bytes"] = 8 * k * row["threads"]
        if cross:
            knn(shuffled), torch.cuda.synchronize()
            row["cross_ms"] = BS.event_ms(lambda: knn(shuffled), REPS)
            knn()                                                               # the outputs are the self query's again
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def kernel_stats(dirname):
    """{kernel: (calls, average ns)} of k_knn_query and k_cl_query in a rocprofv3 --stats directory."""
    import csv
    hits = sorted(glob.glob(os.path.join(dirname, "**", "*kernel_stats.csv"), recursive=True))
    if not hits:
        raise SystemExit(f"no *kernel_stats.csv under {dirname}")
    out = {}
    for r in csv.DictReader(open(hits[0])):
        for key, tag in (("k_knn_query", "knn"), ("k_cl_query", "counts")):
            if key in r["Name"]:
                kind = tag + (" cross" if key == "k_knn_query" and ("true" in r["Name"] or "Lb1E" in r["Name"]) else "")
                calls, ns = out.get(kind, (0, 0.0))
                out[kind] = (calls + int(r["Calls"]), ns + int(r["Calls"]) * float(r["AverageNs"]))
    return {k: (calls, ns / calls) for k, (calls, ns) in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_bench.md"))
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--factor", type=float, default=3.0)
    ap.add_argument("--ks", default="8,16,32")
    ap.add_argument("--variant-lib", default="")
    ap.add_argument("--stats", default="")
    ap.add_argument("--workload", action="store_true", help="run the calls untimed (for a profiler) and write nothing")
    ap.add_argument("--child", action="store_true", help="time the self query with the library of M3SLAM_LIB, print JSON")
    ap.add_argument("--resources-only", action="store_true", help="print the code object's metadata and stop (no device)")
    a = ap.parse_args()
    if a.resources_only:
        print(json.dumps(resources(_ffi.LIB_PATH), indent=1))
        return
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: nothing is measured without one")
    ks = [int(k) for k in a.ks.split(",")]
    radius = float(np.float32(a.factor * a.voxel))
    ab = []
    if a.variant_lib and not (a.child or a.workload):                           # before this process opens the device
        for name, lib in (("A", ""), ("B", a.variant_lib)) * 2:
            env = dict(os.environ, M3SLAM_LIB=lib) if lib else {k: v for k, v in os.environ.items() if k != "M3SLAM_LIB"}
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--voxel", str(a.voxel), "--factor", str(a.factor),
                                "--ks", a.ks], env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"child {name} failed with {r.returncode}:\n{r.stdout}\n{r.stderr}")
            ab.append((name, json.loads(r.stdout.strip().splitlines()[-1])))
            print(name, ab[-1][1], flush=True)
    dev = torch.device("cuda:0")
    p = load_cloud(a.voxel, dev)
    rows = measure(p, radius, ks, cross=not a.child, workload=a.workload)
    if a.workload:
        return
    if a.child:
        print(json.dumps([dict(k=r["k"], knn_ms=r["knn_ms"], sha256=r["sha256"]) for r in rows]))
        return
    stats = {int(k): kernel_stats(d) for k, d in (kv.split("=") for kv in a.stats.split(",") if kv)}
    res = resources(_ffi.LIB_PATH)
    t3 = lambda x: ", ".join(f"{y:.4f}" for y in x)
    M = rows[0]["M"]
    lines = ["# k nearest neighbours within a radius: `cloud.cloud_knn`", "",
             "Tool: `python tools/bench_knn.py` (its docstring says what is timed and how).  "
             f"Device: {torch.cuda.get_device_name(0)} (the library is built for gfx950 alone: an MI355X).  Nothing here is a gate: no "
             "k-NN existed before, and these are the numbers a later change improves on.", "",
             f"Cloud: `collect_map` of 8 keyframes of 512 x 512 that see one surface, one point per voxel of {a.voxel}: {M} points; "
             f"radius {a.factor:g} voxel edges.  Launches: {rows[0]['launches']} for a query whatever the cloud holds - the six of the "
             "index build and one query kernel - as for the counts-only pass.  Times in ms: median, min, max of 5 rounds of "
             f"{REPS} calls; every pair of columns was measured twice in the same job, one after the other, to show the spread.", "",
             "| k | threads per workgroup | LDS per workgroup (dynamic) | `m3_knn_query`, 7 launches, device | again | counts-only "
             "`m3_cloud_neighbors`, 7 launches, device | again | difference: the price of selection | cross mode, the same points "
             "shuffled as queries | rows with k neighbours | identical bytes |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['k']} | {r['threads']} | {r['lds_bytes']} | {t3(r['knn_ms'])} | {t3(r['knn_ms_again'])} | {t3(r['counts_ms'])} | "
                     f"{t3(r['counts_ms_again'])} | {r['knn_ms'][0] - r['counts_ms'][0]:.4f} | {t3(r['cross_ms'])} | "
                     f"{100 * r['complete']:.2f} % | {r['identical_bytes']} |")
    lines += ["", "Kernel times (`rocprofv3 --kernel-trace --stats` around `--workload`, a run of its own per k):", "",
              "| k | kernel | calls | average (ms) |", "|---|---|---|---|"]
    for r in rows:
        if r["k"] not in stats:
            lines.append(f"| {r['k']} | all | - | not measured |")
            continue
        for kind, (calls, ns) in sorted(stats[r["k"]].items()):
            lines.append(f"| {r['k']} | {kind} | {calls} | {ns * 1e-6:.4f} |")
    lines += ["", "Code object metadata (gfx950; scratch must be 0; the k-best list is dynamic LDS, 8 k threads bytes, see above):", "",
              "| kernel | workgroup | VGPR | SGPR | scratch bytes per lane | static LDS bytes |", "|---|---|---|---|---|---|"]
    for name in sorted(res):
        v = res[name]
        lines.append(f"| `{name}` | {v['threads']} | {v['vgpr']} | {v['sgpr']} | {v['scratch']} | {v['lds']} |")
    if ab:
        lines += ["", "## The selection, two ways", "",
                  "A: the shipped list - unordered in LDS, the worst key and its position in registers, a candidate that enters "
                  "overwrites the worst and scans the k words for the new one, one insertion sort at the end.  B: the list kept in "
                  "ascending order - a candidate that enters shifts the larger keys up by one, the worst key is the last entry, no "
                  "final sort (the same file with that loop in place of the overwrite-and-scan, linked with the shipped objects; "
                  "its source is not kept).  Fresh processes alternating A B A B in one job on the same cloud; `m3_knn_query`, 7 launches, device ms "
                  "(median, min, max), and whether index, dist2 and found of the run have the SHA-256 of the first A:", "",
                  "| run | " + " | ".join(f"k = {k}" for k in ks) + " | bytes equal to the first A |", "|---|" + "---|" * (len(ks) + 1)]
        ref = [x["sha256"] for x in ab[0][1]]
        for name, got in ab:
            lines.append(f"| {name} | " + " | ".join(t3(x["knn_ms"]) for x in got) + f" | {[x['sha256'] for x in got] == ref} |")
        med = lambda name, i: float(np.median([got[i]["knn_ms"][0] for n, got in ab if n == name]))
        lines += ["", "B against A, medians of the two runs each: " +
                  ", ".join(f"k = {k}: {100 * (med('B', i) / med('A', i) - 1):+.1f} %" for i, k in enumerate(ks)) +
                  ".  The spread between the two runs of one library is the noise to hold that against.  Not tried: a register "
                  "list for k <= 8; a float32 pre-test of `d2` against the worst key before the float64 one; one wave per cell with "
                  "the candidates staged through LDS; cross queries sorted through an index of their own."]
    lines += ["", "```json", json.dumps(dict(rows=rows, ab=ab, resources=res)), "```", ""]
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
