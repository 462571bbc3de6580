"""Device time of the vertex normals and the lit mesh views, on the two meshes the project produces.

    python tools/bench_normals.py [--out profiles/normals_bench.md] [--cases fused,keyframes]

The meshes are those of tools/bench_components.py.  fused: the default fused mesh of the 256:16 case of
tools/bench_tsdf.py (a cube of 256^3 voxels over 16 keyframes of 512 x 512 that see one surface), beside
fusion.extract_surface on the same volume.  keyframes: export.collect_mesh of 8 keyframes of 512 x 512 at stride 1,
beside collect_mesh itself.

What is timed, median / min / max of 5 rounds after a warm-up:
  * host clock around calls that end in a device synchronise: the producer (with its one host read), vertex_normals and
    shade_vertices as a user calls them (with their allocations);
  * device events around replays of a graph that holds the calls on prebuilt outputs and workspaces: vertex_normals (3
    launches), the same call with F = 0 (the clear and the vertex pass alone; the difference is the face pass),
    shade_vertices (1 launch), render_mesh as it was (4 launches, the parent's code path, shading=None) and the lit
    render_mesh with the normals given (1 + 4 launches), at 480 x 640 from the first keyframe;
  * device events around eager calls of the lit render_mesh that computes the normals itself (3 + 1 + 4 launches and
    three allocations).

The face pass adds 9 int64 values per contributing face: 72 bytes of atomic adds.  Its rate is printed beside about
1.3 TB/s, the chip-wide rate of fp32 global atomic adds on an MI355X when a wave's adds are contiguous; the 64-bit
integer form and this access shape (8-byte words, contiguous only where the vertex rows of neighbouring lanes are) are
not covered by that figure, so it is a yardstick, not a bound.
It also reads 12 F bytes of faces and 36 F bytes of scattered vertices."""
import argparse
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
import normals_twin as NT  # noqa: E402
import render_scenes as RS  # noqa: E402
from mast3r_slam import _ffi, export, fusion, normals, render  # noqa: E402

H = W = 512
ORIGIN, SIDE, D, K_FUSED, K_MESH = (-2.0, -2.0, 0.5), 4.0, 256, 16, 8
VIEW = (480, 640)
ATOMIC_TBS = 1.3
# The first version kept the three sums of a vertex side by side (int64 [V][3]); the same tool measured it before the planes
# (int64 [3][V]) replaced it: (vertex_normals device ms, face pass ms), medians.
SIDE_BY_SIDE = {"fused": (0.0598, 0.0467), "keyframes": (0.1727, 0.1511)}


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


def graphed(call, reps):
    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    g.replay()
    torch.cuda.synchronize()
    return event_ms(g.replay, reps)


def producer(case, dev):
    """(the call that makes the mesh, its name, the keyframes)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_bench.md"))
    ap.add_argument("--cases", default="fused,keyframes")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: nothing is measured without one")
    dev = torch.device("cuda:0")
    rows = []
    for case in a.cases.split(","):
        make, name, frames = producer(case, dev)
        v, c, f = make()[:3]
        V, F = int(v.shape[0]), int(f.shape[0])
        pose = frames[0].T_WC.reshape(-1).to(torch.float32).contiguous().clone()
        Kc = render.scaled_intrinsics(CT.shared_pinhole(H, W), (H, W), VIEW)
        n = normals.vertex_normals(v, f)
        same = n.cpu().numpy().tobytes() == normals.vertex_normals(v, f).cpu().numpy().tobytes()
        vh, fh = v.cpu().numpy(), f.cpu().numpy()
        twin = NT.vertex_normals(vh, fh)
        contributing = int(len(NT.face_contributions(vh, fh)[0]))
        nrm = torch.empty_like(n)
        lit = torch.empty_like(c)
        nws = torch.empty(normals.workspace_bytes(V), dtype=torch.uint8, device=dev)
        out = (torch.empty((*VIEW, 3), dtype=torch.uint8, device=dev), torch.empty(VIEW, dtype=torch.float32, device=dev))
        ws = torch.empty(render.mesh_workspace_bytes(V, VIEW), dtype=torch.uint8, device=dev)
        no_faces = f[:0]
        reps = max(4, min(200, (1 << 25) // max(F, 1)))
        row = dict(case=case, producer=name, V=V, F=F, contributing_faces=contributing, view=list(VIEW),
                   identical_bytes=bool(same), equals_twin=bool(n.cpu().numpy().tobytes() == twin.tobytes()),
                   zero_normals=int((~twin.any(axis=1)).sum()), launches=int(_ffi.lib().m3_mesh_normals_launches()),
                   ws_bytes=int(nws.numel()),
                   producer_ms=host_ms(make, reps),
                   normals_call_ms=host_ms(lambda: normals.vertex_normals(v, f), reps),
                   shade_call_ms=host_ms(lambda: normals.shade_vertices(v, n, c, pose), reps),
                   normals_ms=graphed(lambda: normals.vertex_normals(v, f, out=nrm, workspace=nws), reps),
                   normals_no_faces_ms=graphed(lambda: normals.vertex_normals(v, no_faces, out=nrm, workspace=nws), reps),
                   shade_ms=graphed(lambda: normals.shade_vertices(v, n, c, pose, out=lit), reps),
                   render_plain_ms=graphed(lambda: render.render_mesh(v, c, f, pose, Kc, VIEW, out=out, workspace=ws), reps),
                   render_given_normals_ms=graphed(lambda: render.render_mesh(v, c, f, pose, Kc, VIEW, out=out, workspace=ws,
                                                                              shading="headlight", normals=n), reps))
        torch.cuda.synchronize()
        # the lit call allocates its temporaries (normals, sums, colours), which a capture would pin: timed eagerly
        row["render_lit_ms"] = event_ms(lambda: render.render_mesh(v, c, f, pose, Kc, VIEW, out=out, workspace=ws,
                                                                   shading="headlight"), reps)
        face_ms = row["normals_ms"][0] - row["normals_no_faces_ms"][0]
        row["face_pass_ms"] = face_ms
        row["atomic_bytes"] = 72 * contributing
        row["atomic_tb_per_s"] = 72 * contributing / (face_ms * 1e-3) / 1e12 if face_ms > 0 else None
        rows.append(row)
        print(json.dumps(row), flush=True)
        del frames, make, v, c, f, n, nrm, lit, nws, out, ws
        torch.cuda.empty_cache()
    t3 = lambda x: ", ".join(f"{y:.3f}" for y in x)
    lines = ["# Vertex normals and lit mesh views: `normals.vertex_normals`, `normals.shade_vertices`, `render_mesh(shading=...)`", "",
             "Tool: `python tools/bench_normals.py` (its docstring says what is timed).  "
             f"Device: {torch.cuda.get_device_name(0)}.  Nothing here is a gate.  One thing was tuned, the layout of the sums (last table).", "",
             "Times in ms: median, min, max of 5 rounds.  `call`: a host clock around the Python call as a user makes it, ending "
             f"in a synchronise.  `device`: events around replays of a graph that holds the call.  View: {VIEW[0]} x {VIEW[1]}.", "",
             "| case | V | F | contributing faces | zero normals | producer | producer call with its host read | `vertex_normals` call | "
             "`vertex_normals` device | same with F = 0 | `shade_vertices` call | `shade_vertices` device | identical bytes | equals the twin |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['V']} | {r['F']} | {r['contributing_faces']} | {r['zero_normals']} | `{r['producer']}` | "
                     f"{t3(r['producer_ms'])} | {t3(r['normals_call_ms'])} | {t3(r['normals_ms'])} | {t3(r['normals_no_faces_ms'])} | "
                     f"{t3(r['shade_call_ms'])} | {t3(r['shade_ms'])} | {r['identical_bytes']} | {r['equals_twin']} |")
    lines += ["", "| case | plain `render_mesh` device (the parent's path) | lit, normals given, device | lit, normals computed in the "
              "call, eager with its allocations |", "|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {t3(r['render_plain_ms'])} | {t3(r['render_given_normals_ms'])} | {t3(r['render_lit_ms'])} |")
    lines += ["", f"Face pass = `vertex_normals` device minus the same call with F = 0; 72 bytes of int64 atomic adds per contributing "
              f"face, beside about {ATOMIC_TBS} TB/s for contiguous fp32 atomic adds chip-wide (a yardstick, not a bound for this shape):", "",
              "| case | face pass (ms) | atomic bytes | TB/s of added bytes | share of the yardstick |", "|---|---|---|---|---|"]
    for r in rows:
        rate = r["atomic_tb_per_s"]
        lines.append(f"| {r['case']} | {r['face_pass_ms']:.4f} | {r['atomic_bytes']} | " +
                     (f"{rate:.3f} | {100 * rate / ATOMIC_TBS:.0f} % |" if rate else "- | - |"))
    lines.append("")
    for r in rows:
        lines.append(f"* {r['case']}: `vertex_normals` takes {r['normals_call_ms'][0]:.3f} ms as a call ({r['normals_ms'][0]:.3f} ms on the "
                     f"device) beside {r['producer_ms'][0]:.3f} ms for `{r['producer']}`; the lit view takes {r['render_lit_ms'][0]:.3f} ms "
                     f"beside {r['render_plain_ms'][0]:.3f} ms for the plain one.")
    lines += ["", "Layout of the sums, the one thing that was tuned: the first version kept the three sums of a vertex side by side "
              "(`int64 [V][3]`), the shipped one keeps three planes (`int64 [3][V]`), so that the adds of one wave instruction to "
              "neighbouring rows are contiguous.  Side by side as this tool measured it before the change, planes from this run:", "",
              "| case | `vertex_normals` device, side by side (ms) | planes (ms) | face pass, side by side (ms) | planes (ms) |",
              "|---|---|---|---|---|"]
    for r in rows:
        if r["case"] in SIDE_BY_SIDE:
            old = SIDE_BY_SIDE[r["case"]]
            lines.append(f"| {r['case']} | {old[0]:.4f} | {r['normals_ms'][0]:.4f} | {old[1]:.4f} | {r['face_pass_ms']:.4f} |")
    lines += ["", "Nothing else was tuned: the wave-level sum for a shared row starts at half a wave (32 lanes), a value that was "
              "not measured against others.", "", "```json", json.dumps(rows), "```", ""]
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
