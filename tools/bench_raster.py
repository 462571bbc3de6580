"""Device time of render.render_mesh beside render.render_map of the same keyframes, and the rasteriser's walk threshold.

    python tools/bench_raster.py --build-variants             # no GPU: libraries with M3_RASTER_WALK = 16 and 256
    python tools/bench_raster.py --out profiles/raster_bench.md [--commit TEXT]

Scenes: 8 keyframes of 512 x 512 (tests/render_scenes.general_scene, uint8 images) as the keyframe mesh at stride 1 and
stride 4 (every point kept, edge_ratio 0.1) and as the fused mesh (fusion.fuse_tsdf over the box of the points, 256
voxels along its longest side), and one screen-filling quad of two faces; each at 480 x 640 and 1080 x 1920, camera
inside the map.  Events around 20 replays of a graph that holds one call, median of 5 rounds.  --out gets the table,
and the rows as JSON beside it.

Every measurement runs in a process of its own under its own time limit (the parent never opens the GPU), the shipped
library first and then, through M3SLAM_LIB, the variant builds; the parent stops at the first child that fails."""
import argparse
import json
import os
import platform
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tools", "experiments", "_build")
WALKS = (16, 64, 256)
SIZES = ((480, 640), (1080, 1920))
CHILD_LIMIT_S = 240


def variant_lib(walk):
    return os.path.join(BUILD, f"libm3slam_walk{walk}.so")


def build_variants():
    sys.path.insert(0, os.path.join(ROOT, "mast3r-slam_amd"))
    import build as B
    B.build(verbose=False)
    os.makedirs(BUILD, exist_ok=True)
    others = [os.path.join(B.OUT, s.replace(".hip", ".o")) for s in B._sources() if s != "raster.hip"]
    for walk in WALKS:
        if walk == 64:
            continue                                                            # the shipped library
        obj = os.path.join(BUILD, f"raster_walk{walk}.o")
        for cmd in ([B.HIPCC, *B.COMMON, *B.PER_FILE["raster.hip"], f"-DM3_RASTER_WALK={walk}", "-c", os.path.join(B.SRC, "raster.hip"), "-o", obj],
                    [B.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", variant_lib(walk), *others, obj]):
            subprocess.run(cmd, check=True)
        print(variant_lib(walk))


def child(walk, with_points):
    import numpy as np
    import torch
    for p in (ROOT, os.path.join(ROOT, "mast3r-slam_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import render_scenes as RS
    from mast3r_slam import export, fusion, render

    def timed(fn, reps=20, rounds=5):
        out = []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / reps)
        return float(np.median(out))

    def graphed(call):
        call()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        g.replay()
        torch.cuda.synchronize()
        return timed(g.replay)

    dev = torch.device("cuda:0")
    K, H, W = 8, 512, 512
    sc = RS.general_scene(K, H, W, seed=K, layout="u8")
    frames = RS.frames_of(sc, dev)
    fk = 0.78 * W
    meshes = {"keyframes stride 1": export.collect_mesh(frames, c_conf_threshold=None, stride=1, edge_ratio=0.1),
              "keyframes stride 4": export.collect_mesh(frames, c_conf_threshold=None, stride=4, edge_ratio=0.1)}
    lo, hi = fusion.map_bounds(frames, None)
    voxel = max(float(h) - float(l) for l, h in zip(lo, hi)) / 256.0
    volume = fusion.fuse_tsdf(frames, (fk, fk, (W - 1) / 2, (H - 1) / 2), voxel, bounds=(lo, hi), c_conf_threshold=None)
    meshes["fused, 256 voxels"] = fusion.extract_surface(volume)
    del volume
    quad_v = torch.tensor([[-9, -7, 2.0], [9, -7, 2.5], [-9, 7, 3.0], [9, 7, 3.5]], dtype=torch.float32, device=dev)
    meshes["one quad"] = (quad_v, torch.tensor([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255]], dtype=torch.uint8, device=dev),
                          torch.tensor([[0, 2, 1], [1, 2, 3]], dtype=torch.int32, device=dev))
    tables = render.map_tables(frames)
    for size in SIZES:
        view, Kc = RS.general_view(size, "inside")
        pose = torch.from_numpy(view).to(dev)
        out = (torch.empty((*size, 3), dtype=torch.uint8, device=dev), torch.empty(size, dtype=torch.float32, device=dev),
               torch.empty(size, dtype=torch.int64, device=dev))
        for name, mesh in meshes.items():
            ws = torch.empty(render.mesh_workspace_bytes(mesh[0].shape[0], size), dtype=torch.uint8, device=dev)
            ms = graphed(lambda: render.render_mesh(mesh, pose, Kc, size, near=0.5, return_index=True, out=out, workspace=ws))
            print(json.dumps(dict(walk=walk, what=name, size=list(size), V=int(mesh[0].shape[0]), F=int(mesh[2].shape[0]), ms=ms,
                                  covered=int((out[2] >= 0).sum()))), flush=True)
        if with_points:
            ws = torch.empty(render.workspace_bytes(size), dtype=torch.uint8, device=dev)
            for ps in (1, 3):
                ms = graphed(lambda: render.render_map(tables, pose, Kc, size, near=0.5, c_conf_threshold=None, point_size=ps,
                                                       return_index=True, out=out, workspace=ws))
                print(json.dumps(dict(walk=None, what=f"render_map point_size {ps}", size=list(size), V=K * H * W, F=0, ms=ms,
                                      covered=int((out[2] >= 0).sum()))), flush=True)
    print(json.dumps(dict(box=f"{platform.node()}, {torch.cuda.get_device_name(0)}")), flush=True)


def write_md(path, rows, box, commit):
    cell = lambda what, size, walk: next((r for r in rows if r["what"] == what and r["size"] == list(size) and r["walk"] == walk), None)
    whats = [w for w in dict.fromkeys(r["what"] for r in rows) if not w.startswith("render_map")]
    with open(path, "w") as f:
        f.write("# Triangle rasteriser (tools/bench_raster.py)\n\n")
        f.write(f"Box: {box}.  Commit: {commit}.\n\n")
        f.write("One MI355X, a process per library.  `ms`: device time between events around 20 replays of a graph that holds one\n"
                "`render_mesh` call (clear + project + raster + resolve; rgb + depth + index outputs), median of 5 rounds.  Scene: 8\n"
                "keyframes of 512 x 512 (`tests/render_scenes.general_scene`), every point kept, camera inside the map; the keyframe\n"
                "meshes are `collect_mesh(..., edge_ratio=0.1)`, the fused mesh `fuse_tsdf` at 256 voxels along the longest side of\n"
                "the map's box.  `render_map` of the same keyframes (2.1 M points) is the yardstick.  `walk` is the largest bounding\n"
                "box, in pixels, that a face's own lane walks (`M3_RASTER_WALK`; 64 is the shipped library, the others are builds of\n"
                "`raster.hip` with `-DM3_RASTER_WALK=`).\n\n")
        f.write("| what | V | F | view | covered px | " + " | ".join(f"walk {w} ms" for w in WALKS) + " | walk 64 again ms |\n|---|---|---|---|---|---|" + "---|" * len(WALKS) + "\n")
        for size in SIZES:
            for what in whats:
                r = cell(what, size, 64)
                ms = [cell(what, size, w) for w in WALKS]
                f.write(f"| {what} | {r['V']} | {r['F']} | {size[0]}x{size[1]} | {r['covered']} | "
                        + " | ".join("-" if m is None else f"{m['ms']:.3f}" for m in ms) + f" | {r.get('ms_again', float('nan')):.3f} |\n")
            for r in rows:
                if r["what"].startswith("render_map") and r["size"] == list(size):
                    f.write(f"| {r['what']} | {r['V']} | - | {size[0]}x{size[1]} | {r['covered']} | " + " | ".join(["-", f"{r['ms']:.3f}", "-", f"{r.get('ms_again', float('nan')):.3f}"]) + " |\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-variants", action="store_true")
    ap.add_argument("--child", type=int, default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="working tree")
    a = ap.parse_args()
    if a.build_variants:
        return build_variants()
    if a.child is not None:
        return child(a.child, a.child == 64)
    rows, box = [], "?"
    for walk in (64, 16, 256, 64):                                              # the shipped library twice: the spread
        env = dict(os.environ)
        if walk != 64:
            if not os.path.exists(variant_lib(walk)):
                sys.exit(f"{variant_lib(walk)} is missing: run with --build-variants first")
            env["M3SLAM_LIB"] = variant_lib(walk)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(walk)], env=env, capture_output=True, text=True,
                           timeout=CHILD_LIMIT_S)
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            sys.exit(f"child for walk {walk} failed with {r.returncode}:\n{r.stderr[-2000:]}")
        new = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        box = next((n["box"] for n in new if "box" in n), box)
        new = [n for n in new if "box" not in n]
        if walk == 64 and rows:
            for n in new:                                                       # second run of the shipped library
                first = next(x for x in rows if (x["what"], x["size"], x["walk"]) == (n["what"], n["size"], n["walk"]))
                first["ms_again"] = n["ms"]
        else:
            rows += new
    if a.out:
        write_md(a.out, rows, box, a.commit)
        with open(os.path.splitext(a.out)[0] + ".json", "w") as f:
            json.dump(dict(box=box, commit=a.commit, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
