#!/usr/bin/env python3
"""Map export in isolation (csrc/map_export.hip through export.collect_map), device-event timing of whole calls:
  K in {16, 256} keyframes of 512x512 points, synthetic pointmaps / confidences from a seed, float [3,H,W] images, a
  threshold that keeps about half the points; voxel thinning off and on.
In the same process, the composition a caller had before this path existed: per keyframe m3_sim3_act, torch.cat, a
boolean-mask index of the points and of torch-converted colours.  Both produce the same cloud (checked here).
Writes profiles/map_export_bench.md: times with their spread, the algorithmic bytes over the time, that figure as a
share of the HBM peak (--hbm, TB/s; default 8.0, the MI355X datasheet figure), the voxel table occupancy and the
compile-time resource usage of every kernel (hipcc -Rpass-analysis=kernel-resource-usage; scratch must be zero)."""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mast3r-slam_amd")]
import torch
from mast3r_slam import export
from mast3r_slam.frame import Frame
from mast3r_slam.tracker import sim3_act

HBM = float(sys.argv[sys.argv.index("--hbm") + 1]) if "--hbm" in sys.argv else 8.0
SIZES = [int(v) for v in sys.argv[sys.argv.index("--keyframes") + 1].split(",")] if "--keyframes" in sys.argv else [16, 256]
REPS = 20
H = W = 512
N = H * W
THR, VOXEL = 1.5, 0.05
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "map_export_bench.md")
dev = torch.device("cuda:0")


def scene(K):
    g = torch.Generator(device=dev).manual_seed(K)
    frames = []
    for k in range(K):
        q = torch.randn(4, generator=g, device=dev)
        T = torch.cat([torch.randn(3, generator=g, device=dev), q / q.norm(), torch.tensor([1.2], device=dev)])[None]
        f = Frame(frame_id=k, img=torch.rand(3, H, W, generator=g, device=dev), T_WC=T)
        f.N = 1 + k % 3
        f.X_canon = torch.randn(N, 3, generator=g, device=dev)
        f.C = (0.5 + 2.0 * torch.rand(N, 1, generator=g, device=dev)) * f.N      # average confidence uniform in [0.5, 2.5]
        frames.append(f)
    return frames


def composition(frames):
    pts = torch.cat([sim3_act(f.T_WC, f.X_canon) for f in frames])
    conf = torch.cat([f.C.reshape(-1) / f.N for f in frames])
    col = torch.cat([(f.img.clamp(0, 1) * 255).floor().to(torch.uint8).permute(1, 2, 0).reshape(-1, 3) for f in frames])
    keep = (conf > THR) & torch.isfinite(pts).all(dim=1)
    return pts[keep], col[keep]


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
    src = os.path.join(ROOT, "mast3r-slam_amd", "csrc", "map_export.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17",
                            "-fhip-fp32-correctly-rounded-divide-sqrt", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                            "-o", os.path.join(tmp, "x.o")], capture_output=True, text=True, check=True)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: +(Function Name|VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = re.search(r"k_[a-z_]+", m.group(2)).group(0) + ("<u8>" if "ILi1E" in m.group(2) else "")
            cur = {"name": name}
            rows.append(cur)
        else:
            cur[m.group(1).split(" ")[0]] = m.group(2)
    assert rows and all(r["ScratchSize"] == "0" for r in rows), rows
    return rows


lines = ["# Map export (tools/bench_map_export.py)", "",
         f"Box: {torch.cuda.get_device_name(0)}; device events around whole calls on a warmed stream, {REPS} repetitions, "
         f"median (min - max).  {H}x{W} points per keyframe, float [3,H,W] images, threshold {THR} on average confidences "
         "uniform in [0.5, 2.5] (keeps about half).  `collect_map` includes its one device-to-host read of the kept count.  "
         "'bytes' are the algorithmic ones: the count pass reads C (4 B per point) and X (12 B) of the points that pass the "
         "confidence test, the scatter pass reads 28 B per point and writes 15 B per kept point.  The composition is the path "
         f"a caller had before: per keyframe `m3_sim3_act`, `torch.cat`, boolean-mask index of points and of "
         f"torch-converted colours.  HBM reference {HBM} TB/s.", "",
         "| keyframes | points | kept | collect_map ms | composition ms | speed-up | GB moved | GB/s | of HBM |",
         "|---|---|---|---|---|---|---|---|---|"]
vox = ["", f"Voxel thinning (`voxel_size = {VOXEL}`, on top of the rows above; no comparison exists):", "",
       "| keyframes | input points | voxels kept | collect_map ms (thinning on) | table slots | occupancy |", "|---|---|---|---|---|---|"]
for K in SIZES:
    frames = scene(K)
    p, c = export.collect_map(frames, c_conf_threshold=THR)
    pr, cr = composition(frames)
    assert p.shape == pr.shape and float((p - pr).abs().max()) < 1e-5 and torch.equal(c, cr), "the two paths disagree"
    m = p.shape[0]
    del p, c, pr, cr
    a, b = [], []
    for _ in range(2):                                                    # alternate the two paths
        a.append(timed(lambda: export.collect_map(frames, c_conf_threshold=THR)))
        b.append(timed(lambda: composition(frames)))
    f_med, f_min, f_max = min(x[0] for x in a), min(x[1] for x in a), max(x[2] for x in a)
    c_med, c_min, c_max = min(x[0] for x in b), min(x[1] for x in b), max(x[2] for x in b)
    nbytes = K * N * (4 + 28) + m * (12 + 15)
    gbs = nbytes / f_med / 1e6
    row = (f"| {K} | {K * N} | {m} | {f_med:.3f} ({f_min:.3f} - {f_max:.3f}) | {c_med:.3f} ({c_min:.3f} - {c_max:.3f}) | "
           f"{c_med / f_med:.2f}x | {nbytes / 1e9:.3f} | {gbs:.0f} | {gbs / (HBM * 1e3):.2f} |")
    print(row, flush=True)
    lines.append(row)
    v_med, v_min, v_max = timed(lambda: export.collect_map(frames, c_conf_threshold=THR, voxel_size=VOXEL))
    st = export.last_voxel_stats
    row = (f"| {K} | {st['points']} | {st['voxels']} | {v_med:.3f} ({v_min:.3f} - {v_max:.3f}) | {st['slots']} | "
           f"{st['voxels'] / st['slots']:.3f} |")
    print(row, flush=True)
    vox.append(row)
    del frames
    torch.cuda.empty_cache()
res = ["", "Compile-time resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; scratch is zero everywhere):", "",
       "| kernel | VGPRs | SGPRs | LDS bytes | scratch bytes/lane | waves/SIMD |", "|---|---|---|---|---|---|"]
res += [f"| `{r['name']}` | {r['VGPRs']} | {r['TotalSGPRs']} | {r['LDS']} | {r['ScratchSize']} | {r['Occupancy']} |"
        for r in resources()]
with open(OUT, "w") as f:
    f.write("\n".join(lines + vox + res) + "\n")
print("wrote", OUT)
