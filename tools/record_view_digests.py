"""SHA-256 of the outputs - and of every input array - of the view passes (render_map, render_mesh, multiview_support,
fuse_tsdf and their C entry points) on small deterministic cases, for tests/test_gpu_view_family.py.

    python tools/record_view_digests.py            # rewrites tests/golden/view_family_digests.json (needs the device)

The committed file was recorded once with the library of the commit before the view passes were folded onto
csrc/view_dev.h and cons_planes.h (M3SLAM_LIB names the library); the test recomputes it at the tree.  The
cases are the smallest at which each shared part can go wrong: a view of 61 x 83 (P % 4 = 3), of 8 x 8 (P % 4 = 0) and
of 1 x 5 (one thread, tail only), outputs carved at odd offsets (the scalar paths), N % 4 = 0 and != 0, an empty map, an
empty mesh, a workspace that holds 0xa5, and an infinite principal point through the C entry points."""
from __future__ import annotations

import hashlib
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "mast3r-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import consistency_twin as CT  # noqa: E402
import raster_scenes as RA  # noqa: E402
import render_scenes as RS  # noqa: E402
import tsdf_twin as TT  # noqa: E402
from mast3r_slam import _ffi, consistency, fusion, render  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "view_family_digests.json")
VIEWS = ((61, 83), (8, 8), (1, 5))
INF = math.inf


def sha(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        h.update(f"{a.dtype} {a.shape} ".encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def scene_arrays(sc):
    return [sc[k] for k in ("X", "C", "Nk", "T", "img")]


def dirty(nbytes, dev):
    return torch.full((nbytes,), 0xa5, dtype=torch.uint8, device=dev)


def carved(size, dev, index=True):
    """rgb, depth and index at odd offsets of larger buffers: none of them 4- or 16-byte aligned."""
    hv, wv = size
    P = hv * wv
    out = (torch.zeros(3 * P + 1, dtype=torch.uint8, device=dev)[1:].view(hv, wv, 3),
           torch.zeros(P + 1, dtype=torch.float32, device=dev)[1:].view(hv, wv),
           torch.zeros(P + 1, dtype=torch.int64, device=dev)[1:].view(hv, wv))
    return out if index else out[:2]


def render_map_cases(dev, inputs, outputs):
    for layout in ("f32", "u8"):
        for size in VIEWS:
            sc, view, Kc = RS.exact_scene(3, 1023, seed=5, layout=layout, size=size)
            tag = f"render_map {layout} {size[0]}x{size[1]}"
            inputs[tag] = sha(*scene_arrays(sc), np.asarray(view), np.asarray(Kc, dtype=np.float64))
            frames = RS.frames_of(sc, dev)
            view_t = torch.from_numpy(np.asarray(view, dtype=np.float32)).to(dev)
            kw = dict(near=0.125, background=(7, 8, 9))
            for ps in ((1, 7) if size == VIEWS[0] else (1,)):
                for ri in (False, True):
                    ws = dirty(render.workspace_bytes(size), dev)
                    out = render.render_map(frames, view_t, Kc, size, point_size=ps, return_index=ri, workspace=ws, **kw)
                    outputs[f"{tag} ps{ps} index{int(ri)}"] = sha(*out)
            if size == VIEWS[0]:
                out = render.render_map(frames, view_t, Kc, size, point_size=3, return_index=True, out=carved(size, dev), **kw)
                outputs[f"{tag} carved"] = sha(*out)
                outputs[f"{tag} far"] = sha(*render.render_map(frames, view_t, Kc, size, far=4.0, return_index=True, **kw))
                outputs[f"{tag} empty map"] = sha(*render.render_map([], view_t, Kc, size, return_index=True, **kw))


def render_mesh_cases(dev, inputs, outputs):
    for size in VIEWS:
        sc = RA.exact(size, 37, seed=3, shared=True)
        tag = f"render_mesh {size[0]}x{size[1]}"
        inputs[tag] = sha(sc["vertices"], sc["colors"], sc["faces"], sc["view"], np.asarray(sc["K"], dtype=np.float64))
        v, c, f = (torch.from_numpy(sc[k]).to(dev) for k in ("vertices", "colors", "faces"))
        view_t = torch.from_numpy(sc["view"]).to(dev)
        for cull in ("none", "back"):
            ws = dirty(render.mesh_workspace_bytes(v.shape[0], size), dev)
            out = render.render_mesh(v, c, f, view_t, sc["K"], size, cull=cull, return_index=True, workspace=ws, **sc["kw"])
            outputs[f"{tag} cull {cull}"] = sha(*out)
        if size == VIEWS[0]:
            out = render.render_mesh(v, c, f, view_t, sc["K"], size, return_index=True, out=carved(size, dev), **sc["kw"])
            outputs[f"{tag} carved"] = sha(*out)
            outputs[f"{tag} F=0"] = sha(*render.render_mesh(v, c, f[:0], view_t, sc["K"], size, return_index=True, **sc["kw"]))
            outputs[f"{tag} V=0"] = sha(*render.render_mesh(v[:0], c[:0], f, view_t, sc["K"], size, return_index=True, **sc["kw"]))


def consistency_cases(dev, inputs, outputs):
    sc, pin, nbr = CT.exact_scene(seed=4)                               # N = 33 * 65: N % 4 = 1
    inputs["consistency exact"] = sha(*scene_arrays(sc), np.asarray(pin), nbr)
    frames = RS.frames_of(sc, dev)
    kw = dict(depth_rtol=CT.EXACT_RTOL, z_min=CT.EXACT_ZMIN)
    table = torch.from_numpy(nbr).to(dev)                               # holds -1, an own index and an index beyond K
    for label, extra in (("all", dict(neighbours=None)), ("table", dict(neighbours=table)),
                         ("table no limit", dict(neighbours=table, max_conflicts=None)),
                         ("table no threshold", dict(neighbours=table, c_conf_threshold=None)),
                         ("nearest 2", dict(neighbours=2))):
        ws = dirty(consistency.workspace_bytes(sc["K"], sc["N"]), dev)
        outputs[f"consistency exact {label}"] = sha(*consistency.multiview_support(frames, pin, workspace=ws, **kw, **extra))
    outputs["consistency exact alone"] = sha(*consistency.multiview_support(frames[:1], pin, **kw))
    K, H, W, seed = CT.SHARED[0]                                        # a scene on which table and threshold change the counts
    sc, pin = CT.shared_scene(K, H, W, seed), CT.shared_pinhole(H, W)
    table = CT.explicit_table(K)                                        # -1 padding, a row naming itself, a row of only -1
    inputs["consistency shared"] = sha(*scene_arrays(sc), np.asarray(pin), table)
    frames, table = RS.frames_of(sc, dev), torch.from_numpy(table).to(dev)
    for label, extra in (("all", dict(neighbours=None)), ("table", dict(neighbours=table)),
                         ("all no threshold", dict(neighbours=None, c_conf_threshold=None))):
        outputs[f"consistency shared {label}"] = sha(*consistency.multiview_support(frames, pin, **extra))
    sc, pin, _, _ = CT.hand_case()                                      # N = 4: the 16-byte path
    inputs["consistency hand"] = sha(*scene_arrays(sc), np.asarray(pin))
    frames = RS.frames_of(sc, dev)
    outputs["consistency hand"] = sha(*consistency.multiview_support(frames, pin, neighbours=None))
    for label, limit in (("limit 0", 0), ("no limit", None)):           # min_views 0: the conflict limit alone decides
        out = consistency.multiview_support(frames, pin, neighbours=None, min_views=0, max_conflicts=limit)
        outputs[f"consistency hand views 0 {label}"] = sha(*out)


def volume_digest(v):
    return sha(v.tsdf, v.weight, v.color, v.colored)


def fusion_cases(dev, inputs, outputs):
    sc, pin, vol, _, _, _ = TT.hand_case()
    inputs["fusion hand"] = sha(*scene_arrays(sc), np.asarray(pin), vol["origin"])
    out = fusion.empty_volume(vol["origin"], vol["dims"], vol["vs"], vol["trunc"], dev)
    outputs["fusion hand"] = volume_digest(fusion.fuse_tsdf(RS.frames_of(sc, dev), pin, vol["vs"], trunc=vol["trunc"], out=out))
    K, H, W, seed = CT.SHARED[0]
    vol = TT.VOLUME
    for layout in ("u8", "f32"):
        sc, pin = CT.shared_scene(K, H, W, seed, layout=layout), CT.shared_pinhole(H, W)
        inputs[f"fusion shared {layout}"] = sha(*scene_arrays(sc), np.asarray(pin), vol["origin"])
        out = fusion.empty_volume(vol["origin"], vol["dims"], vol["vs"], vol["trunc"], dev)
        ws = dirty(fusion.workspace_bytes(K, H * W), dev)
        v = fusion.fuse_tsdf(RS.frames_of(sc, dev), pin, vol["vs"], trunc=vol["trunc"], out=out, workspace=ws)
        outputs[f"fusion shared {layout}"] = volume_digest(v)
    v = fusion.fuse_tsdf([], pin, 0.25, bounds=((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
    outputs["fusion empty map"] = volume_digest(v)


def infinite_centre_cases(dev, inputs, outputs):
    """cx = +inf through the C entry points: the renderers draw the background, the other two reject it and write nothing."""
    L = _ffi.lib()
    st = _ffi.stream_ptr()
    size = (5, 7)
    sc, view, Kc = RS.exact_scene(3, 1023, seed=5, layout="u8", size=size)
    m = render.map_tables(RS.frames_of(sc, dev))
    view_t = torch.from_numpy(np.asarray(view, dtype=np.float32)).to(dev)
    rgb, depth = torch.zeros((*size, 3), dtype=torch.uint8, device=dev), torch.zeros(size, dtype=torch.float32, device=dev)
    ws = dirty(render.workspace_bytes(size), dev)
    rc = L.m3_render_map(_ffi.ptr(m.table[0]), _ffi.ptr(m.table[1]), _ffi.ptr(m.table[2]), _ffi.ptr(m.poses), _ffi.ptr(m.nk), m.k,
                         m.n, 1, 1.5, m.layout, _ffi.ptr(view_t), Kc[0], Kc[1], INF, Kc[3], size[0], size[1], 0.125, INF, 1, 7, 8,
                         9, _ffi.ptr(ws), ws.numel(), _ffi.ptr(rgb), _ffi.ptr(depth), None, st)
    outputs["m3_render_map cx=inf"] = f"{rc} " + sha(rgb, depth)
    ra = RA.exact(size, 0, seed=3, shared=True)
    v, c, f = (torch.from_numpy(ra[k]).to(dev) for k in ("vertices", "colors", "faces"))
    rview = torch.from_numpy(ra["view"]).to(dev)
    ws = dirty(render.mesh_workspace_bytes(v.shape[0], size), dev)
    rgb.zero_(), depth.zero_()
    rc = L.m3_raster_mesh(_ffi.ptr(v), _ffi.ptr(c), _ffi.ptr(f), v.shape[0], f.shape[0], _ffi.ptr(rview), 64.0, 64.0, INF, 2.0,
                          size[0], size[1], 0.5, INF, 0, 7, 8, 9, _ffi.ptr(ws), ws.numel(), _ffi.ptr(rgb), _ffi.ptr(depth), None, st)
    outputs["m3_raster_mesh cx=inf"] = f"{rc} " + sha(rgb, depth)
    cs, pin, _, _ = CT.hand_case()
    cm = render.map_tables(RS.frames_of(cs, dev))
    k, n = cm.k, cm.n
    sup, con = dirty(k * n, dev).view(k, n), dirty(k * n, dev).view(k, n)
    conf = torch.full((k, n), 5.0, dtype=torch.float32, device=dev)
    nbr = torch.from_numpy(CT.all_others(k)).to(dev)
    ws = dirty(consistency.workspace_bytes(k, n), dev)
    rc = L.m3_consistency(_ffi.ptr(cm.table[0]), _ffi.ptr(cm.table[1]), _ffi.ptr(cm.poses), _ffi.ptr(cm.nk), k, 2, 2, 1, 1.5, 1.0,
                          1.0, INF, 0.5, _ffi.ptr(nbr), nbr.shape[1], 1e-3, 0.03, 2, 1, _ffi.ptr(ws), ws.numel(), _ffi.ptr(sup),
                          _ffi.ptr(con), _ffi.ptr(conf), st)
    outputs["m3_consistency cx=inf"] = f"{rc} " + sha(sup, con, conf, ws)
    vol = fusion.empty_volume((-0.5, -0.5, 1.5), (2, 2, 2), 0.5, 0.5, dev)
    for t in (vol.tsdf, vol.weight, vol.color, vol.colored):
        t.fill_(3)
    rc = L.m3_tsdf_integrate(_ffi.ptr(cm.table[0]), _ffi.ptr(cm.table[1]), _ffi.ptr(cm.table[2]), _ffi.ptr(cm.poses),
                             _ffi.ptr(cm.nk), k, 2, 2, 1, 1.5, cm.layout, 1.0, 1.0, INF, 0.5, 1e-3, -0.5, -0.5, 1.5, 0.5, 0.5, 2, 2,
                             2, _ffi.ptr(ws), ws.numel(), _ffi.ptr(vol.tsdf), _ffi.ptr(vol.weight), _ffi.ptr(vol.color),
                             _ffi.ptr(vol.colored), st)
    outputs["m3_tsdf_integrate cx=inf"] = f"{rc} " + sha(vol.tsdf, vol.weight, vol.color, vol.colored, ws)


def compute(dev="cuda") -> dict:
    """{"inputs": {case: digest}, "outputs": {case: digest}} of every case, run on `dev`."""
    inputs, outputs = {}, {}
    for cases in (render_map_cases, render_mesh_cases, consistency_cases, fusion_cases, infinite_centre_cases):
        cases(dev, inputs, outputs)
    torch.cuda.synchronize()
    return dict(inputs=inputs, outputs=outputs)


if __name__ == "__main__":
    got = compute()
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with open(path, "w") as fh:
        json.dump(got, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{len(got['inputs'])} input and {len(got['outputs'])} output digests -> {path}")
