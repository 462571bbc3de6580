#!/usr/bin/env python3
"""Mesh export in isolation (csrc/mesh.hip through export.collect_mesh), device-event timing of whole calls:
  K in {16, 256} keyframes of 512x512 points, stride 1 and 4, on a smooth synthetic surface with steps: a pinhole with
  f = W looking at a tilted plane near z = 2 with 24x24-pixel blocks near z = 1 on a 64-pixel lattice, confidences
  uniform in [0.5, 2.5] per 32x32-pixel patch (about half the patches pass the threshold), float [3,H,W] images.
The yardstick is export.collect_map on the same scene, in the same process, alternating with the mesh call.
Writes profiles/mesh_bench.md: times with their spread, collect_mesh as a multiple of collect_map, the algorithmic bytes
over the time, that figure as a share of the HBM peak (--hbm, TB/s; default 8.0, the MI355X datasheet figure) and the
compile-time resource usage of every kernel (hipcc -Rpass-analysis=kernel-resource-usage; scratch must be zero)."""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mast3r-slam_amd")]
import torch
from mast3r_slam import export
from mast3r_slam.frame import Frame

HBM = float(sys.argv[sys.argv.index("--hbm") + 1]) if "--hbm" in sys.argv else 8.0
SIZES = [int(v) for v in sys.argv[sys.argv.index("--keyframes") + 1].split(",")] if "--keyframes" in sys.argv else [16, 256]
STRIDES = [1, 4]
REPS = 20
H = W = 512
N = H * W
THR = 1.5
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "mesh_bench.md")
dev = torch.device("cuda:0")


def scene(K):
    g = torch.Generator(device=dev).manual_seed(K)
    v, u = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32),
                          indexing="ij")
    ray = torch.stack([(u - (W - 1) / 2) / W, (v - (H - 1) / 2) / W, torch.ones_like(u)], dim=-1)
    block = ((u.long() % 64) < 24) & ((v.long() % 64) < 24)
    frames = []
    for k in range(K):
        tilt = (torch.rand(2, generator=g, device=dev) - 0.5) * 0.6
        z = torch.where(block, 1.0 + 0.05 * u / W, 2.0 + tilt[0] * (u / W - 0.5) + tilt[1] * (v / W - 0.5))
        q = torch.randn(4, generator=g, device=dev)
        T = torch.cat([torch.randn(3, generator=g, device=dev), q / q.norm(), torch.tensor([1.2], device=dev)])[None]
        f = Frame(frame_id=k, img=torch.rand(3, H, W, generator=g, device=dev), T_WC=T)
        f.N = 1 + k % 3
        f.X_canon = (z[..., None] * ray).reshape(N, 3).contiguous()
        patch = 0.5 + 2.0 * torch.rand(H // 32, W // 32, generator=g, device=dev)
        f.C = (patch.repeat_interleave(32, 0).repeat_interleave(32, 1).reshape(N, 1) * f.N).contiguous()
        frames.append(f)
    return frames


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def resources():
    src = os.path.join(ROOT, "mast3r-slam_amd", "csrc", "mesh.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17",
                            "-fhip-fp32-correctly-rounded-divide-sqrt", "-ffp-contract=off",
                            "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "x.o")],
                           capture_output=True, text=True, check=True)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: +(Function Name|VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = re.search(r"k_[a-z_]+", m.group(2)).group(0)
            name += {"ILb1E": "<dense>", "ILb0E": "<strided>", "ILi0E": "<f32>", "ILi1E": "<u8>"}.get(
                (re.search(r"IL[bi][01]E", m.group(2)) or [""])[0], "")
            cur = {"name": name}
            rows.append(cur)
        else:
            cur[m.group(1).split(" ")[0]] = m.group(2)
    assert rows and all(r["ScratchSize"] == "0" for r in rows), rows
    return rows


lines = ["# Mesh export (tools/bench_mesh.py)", "",
         f"Box: {torch.cuda.get_device_name(0)}; device events around whole calls on a warmed stream, {REPS} repetitions, "
         f"median (min - max), the two paths alternating.  {H}x{W} points per keyframe: a tilted plane near z = 2 with "
         "24x24-pixel blocks near z = 1 every 64 pixels, float [3,H,W] images, average confidences uniform in [0.5, 2.5] "
         f"per 32x32 patch against the threshold {THR}, `edge_ratio` at its default 0.02 * stride.  Both calls include "
         "their one device-to-host read.  `collect_map` is the yardstick: the same scene, same box, same run.  'bytes' are "
         "the algorithmic ones.  collect_map: 32 B per point and 27 B per kept point (profiles/map_export_bench.md).  "
         "collect_mesh, per grid vertex: C 4 B and X 12 B read once by the cell pass; per cell: 1 B of flags written and "
         "read three times (used-vertex count, vertex scatter, face scatter); per emitted vertex: X 12 B and the image "
         "12 B read, 12 + 3 B written, 4 B of remap written and about 4 B read; per kept face 12 B written.  "
         f"HBM reference {HBM} TB/s.", "",
         "| keyframes | stride | grid vertices | V | F | kept of candidates | collect_mesh ms | collect_map ms | multiple | "
         "GB moved | GB/s | of HBM |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
for K in SIZES:
    frames = scene(K)
    for s in STRIDES:
        v, c, f = export.collect_mesh(frames, c_conf_threshold=THR, stride=s)
        nv, nf = v.shape[0], f.shape[0]
        assert nf > 0 and int(f.max()) == nv - 1 and int(f.min()) == 0
        del v, c, f
        hg, wg = -(-H // s), -(-W // s)
        a, b = [], []
        for _ in range(2):                                                    # alternate the two paths
            a.append(timed(lambda: export.collect_mesh(frames, c_conf_threshold=THR, stride=s)))
            b.append(timed(lambda: export.collect_map(frames, c_conf_threshold=THR)))
        m_med, m_min, m_max = min(x[0] for x in a), min(x[1] for x in a), max(x[2] for x in a)
        c_med, c_min, c_max = min(x[0] for x in b), min(x[1] for x in b), max(x[2] for x in b)
        cells = K * (hg - 1) * (wg - 1)
        nbytes = K * hg * wg * 16 + cells * 4 + nv * (24 + 15 + 8) + nf * 12
        gbs = nbytes / m_med / 1e6
        row = (f"| {K} | {s} | {K * hg * wg} | {nv} | {nf} | {nf / (2 * cells):.2f} | {m_med:.3f} ({m_min:.3f} - {m_max:.3f}) | "
               f"{c_med:.3f} ({c_min:.3f} - {c_max:.3f}) | {m_med / c_med:.2f}x | {nbytes / 1e9:.3f} | {gbs:.0f} | "
               f"{gbs / (HBM * 1e3):.2f} |")
        print(row, flush=True)
        lines.append(row)
    del frames
    torch.cuda.empty_cache()
res = ["", "Compile-time resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; scratch is zero everywhere):", "",
       "| kernel | VGPRs | SGPRs | LDS bytes | scratch bytes/lane | waves/SIMD |", "|---|---|---|---|---|---|"]
res += [f"| `{r['name']}` | {r['VGPRs']} | {r['TotalSGPRs']} | {r['LDS']} | {r['ScratchSize']} | {r['Occupancy']} |"
        for r in resources()]
with open(OUT, "w") as f:
    f.write("\n".join(lines + res) + "\n")
print("wrote", OUT)
