"""Device time of the cloud registration: register.register_clouds and its accumulate kernel beside the k = 1 cross query of
the same library, on the cloud of tools/bench_cloud.py and tools/bench_knn.py.

    python tools/bench_icp.py [--out profiles/icp_bench.md] [--voxel 0.01] [--factor 5]
    python tools/bench_icp.py --resources-only          (the code object's metadata, no device)

The target is export.collect_map of the keyframes of tools/bench_simplify.py (8 keyframes of 512 x 512 that see one
surface), thinned to one point per voxel; the source is the whole target moved by a small Sim(3) (0.2 degrees about the
centroid, 0.3 voxel edges, scale 1.004) and rounded to float32; the radius is 5 voxel edges, the README's recipe.

Times: device events around eager calls of the entry points on a prebuilt workspace, 20 calls per round, median, min and
max of 5 rounds after a warm-up.  m3_icp_register is timed at 0, 10 and 30 iterations with tol = 0, so that no iteration
is skipped; the time per iteration is (t30 - t10) / 20, and t0 is the index build plus the evaluation.  m3_icp_sums (the
six index launches, one accumulate, one reduction) is timed beside m3_knn_query in cross mode at k = 1 on the same
queries (the six index launches and one query kernel): at the identity pose the query of a source row is the row itself,
both kernels visit the same candidates in the same order, and the difference is the price of the terms, the tree and the
one-workgroup reduction launch.

Registers, scratch and LDS come from the metadata of the gfx950 code object inside the library."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mast3r-slam_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import bench_knn as BK  # noqa: E402  (the cloud and the code-object reader)
import bench_simplify as BS  # noqa: E402  (the timers)
from mast3r_slam import _ffi, cloud, register  # noqa: E402

REPS = 20


def resources(lib_path):
    import glob
    import re
    import shutil
    import subprocess
    import tempfile
    tmp = tempfile.mkdtemp(prefix="icp_co_")
    try:
        lib = shutil.copy(lib_path, tmp)
        subprocess.run([os.path.join(BK.LLVM, "llvm-objdump"), "--offloading", lib], check=True, capture_output=True, cwd=tmp)
        out = {}
        for co in glob.glob(os.path.join(tmp, "*gfx950*")):
            notes = subprocess.run([os.path.join(BK.LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                                   text=True).stdout
            for block in notes.split("  - .agpr_count")[1:]:
                get = lambda key: re.search(r"^\s{4}\.%s:\s+(\S+)" % key, block, re.M).group(1)
                m = re.search(r"(k_icp_accumulate)ILi([01])E|(k_icp_step)|(k_knn_query)ILi256ELb1E", get("name"))
                if not m:
                    continue
                tag = (f"k_icp_accumulate<{'point_to_plane' if m.group(2) == '1' else 'point_to_point'}>" if m.group(1) else
                       "k_icp_step" if m.group(3) else "k_knn_query<256, cross>")
                out[tag] = dict(threads=int(get("max_flat_workgroup_size")), vgpr=int(get("vgpr_count")), sgpr=int(get("sgpr_count")),
                                scratch=int(get("private_segment_fixed_size")), lds=int(get("group_segment_fixed_size")))
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def moved_copy(p, voxel):
    host = p.cpu().numpy().astype(np.float64)
    g = np.random.default_rng(5)
    axis = g.normal(size=3)
    axis /= np.linalg.norm(axis)
    th = math.radians(0.2)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = 1.004 * (np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K)
    t = g.normal(size=3)
    c = host.mean(axis=0)
    t = c - R @ c + t * 0.3 * voxel / np.linalg.norm(t)
    return torch.from_numpy((host @ R.T + t).astype(np.float32)).to(p.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_bench.md"))
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--factor", type=float, default=5.0)
    ap.add_argument("--resources-only", action="store_true", help="print the code object's metadata and stop (no device)")
    a = ap.parse_args()
    if a.resources_only:
        print(json.dumps(resources(_ffi.LIB_PATH), indent=1))
        return
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: nothing is measured without one")
    dev = torch.device("cuda:0")
    target = BK.load_cloud(a.voxel, dev)
    M = int(target.shape[0])
    radius = float(np.float32(a.factor * a.voxel))
    normals = cloud.cloud_normals(target, 3 * a.voxel)
    source = moved_copy(target, a.voxel)
    st = _ffi.stream_ptr()
    import ctypes
    ident = (ctypes.c_double * 13)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1)
    pose = ctypes.addressof(ident)
    rows = []
    for mode, method in enumerate(("point_to_point", "point_to_plane")):
        row = dict(method=method, M=M, radius=radius)
        for it in (0, 10, 30):
            ws = torch.empty(register.registration_workspace_bytes(M, M, it), dtype=torch.uint8, device=dev)
            call = lambda: _ffi.call("m3_icp_register", _ffi.ptr(source), M, _ffi.ptr(target), _ffi.ptr(normals), M, radius, mode, pose,
                                     1, it, 0.0, 16, None, _ffi.ptr(ws), ws.numel(), st)
            call(), torch.cuda.synchronize()
            row[f"register_{it}_ms"] = BS.event_ms(call, REPS)
            reg = register.read_registration(ws, M, M, it)
            row[f"ran_{it}"], row[f"status_{it}"], row[f"fitness_{it}"] = reg.iterations, reg.status, reg.fitness
            row[f"launches_{it}"] = int(_ffi.lib().m3_icp_launches(it))
        row["per_iteration_ms"] = (row["register_30_ms"][0] - row["register_10_ms"][0]) / 20
        a1 = register.register_clouds(source, target, radius, normals, method, with_scale=True, tol=0.0)
        a2 = register.register_clouds(source, target, radius, normals, method, with_scale=True, tol=0.0)
        row["identical_bytes"] = a1.T.tobytes() == a2.T.tobytes() and a1.history.tobytes() == a2.history.tobytes()
        row["rmse_30"] = a1.inlier_rmse
        # the accumulate beside the k = 1 cross query on the same queries
        ws = torch.empty(register.registration_workspace_bytes(M, M, 0), dtype=torch.uint8, device=dev)
        out = torch.empty((39,), dtype=torch.float64, device=dev)
        sums = lambda: _ffi.call("m3_icp_sums", _ffi.ptr(source), M, _ffi.ptr(target), _ffi.ptr(normals), M, radius, mode, pose,
                                 out.data_ptr(), out.data_ptr() + 24, None, _ffi.ptr(ws), ws.numel(), st)
        index = torch.empty((M, 1), dtype=torch.int32, device=dev)
        dist2 = torch.empty((M, 1), dtype=torch.float32, device=dev)
        found = torch.empty((M,), dtype=torch.int32, device=dev)
        knn = lambda: _ffi.call("m3_knn_query", _ffi.ptr(target), M, radius, _ffi.ptr(source), M, 1, _ffi.ptr(index), _ffi.ptr(dist2),
                                _ffi.ptr(found), _ffi.ptr(ws), ws.numel(), st)
        sums(), knn(), torch.cuda.synchronize()
        row["sums_ms"], row["knn1_ms"] = BS.event_ms(sums, REPS), BS.event_ms(knn, REPS)
        row["sums_ms_again"], row["knn1_ms_again"] = BS.event_ms(sums, REPS), BS.event_ms(knn, REPS)
        row["pairs"] = int(out[:1].view(torch.int64).item())
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = resources(_ffi.LIB_PATH)
    t3 = lambda x: ", ".join(f"{y:.4f}" for y in x)
    lines = ["# Cloud registration: `register.register_clouds`", "",
             "Tool: `python tools/bench_icp.py` (its docstring says what is timed and how).  "
             f"Device: {torch.cuda.get_device_name(0)} (the library is built for gfx950 alone: an MI355X).  Nothing here is a gate: no "
             "registration existed before, and these are the numbers a later change improves on.", "",
             f"Target: `collect_map` of 8 keyframes of 512 x 512 that see one surface, one point per voxel of {a.voxel}: {M} points; the "
             f"source is the whole target moved by a small Sim(3); radius {a.factor:g} voxel edges; with scale; tol = 0 so that every "
             f"iteration runs.  Times in ms: median, min, max of 5 rounds of {REPS} calls.", "",
             "| method | launches at 0 / 10 / 30 iterations | `m3_icp_register`, 0 iterations | 10 iterations | 30 iterations | per "
             "iteration (t30 - t10) / 20 | iterations run, status at 30 | fitness, rmse at 30 | identical bytes |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['method']} | {r['launches_0']} / {r['launches_10']} / {r['launches_30']} | {t3(r['register_0_ms'])} | "
                     f"{t3(r['register_10_ms'])} | {t3(r['register_30_ms'])} | {r['per_iteration_ms']:.4f} | {r['ran_30']}, {r['status_30']} | "
                     f"{r['fitness_30']:.4f}, {r['rmse_30']:.3e} | {r['identical_bytes']} |")
    lines += ["", "The accumulate beside the k = 1 cross query on the same queries (identity pose: the source rows themselves), each "
              "measured twice in the same job to show the spread:", "",
              "| method | `m3_icp_sums`, 8 launches | again | `m3_knn_query` cross, k = 1, 7 launches | again | difference: terms, tree, "
              "reduction launch | contributing pairs |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['method']} | {t3(r['sums_ms'])} | {t3(r['sums_ms_again'])} | {t3(r['knn1_ms'])} | {t3(r['knn1_ms_again'])} | "
                     f"{r['sums_ms'][0] - r['knn1_ms'][0]:.4f} | {r['pairs']} |")
    lines += ["", "Code object metadata (gfx950; scratch must be 0):", "",
              "| kernel | workgroup | VGPR | SGPR | scratch bytes per lane | static LDS bytes |", "|---|---|---|---|---|---|"]
    for name in sorted(res):
        v = res[name]
        lines.append(f"| `{name}` | {v['threads']} | {v['vgpr']} | {v['sgpr']} | {v['scratch']} | {v['lds']} |")
    lines += ["", "Not tried: source rows sorted through the target's cells (the lanes of a wave would share cells, as in the self "
              "query); DPP row operations in place of the xor shuffles; the reduction of the 36 sums by `m3_block_reduce36`'s LDS "
              "columns, which has another summation order and would change the rule.",
              "", "```json", json.dumps(dict(rows=rows, resources=res)), "```", ""]
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
