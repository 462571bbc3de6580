"""GPU: vertex normals and lit vertex colours (csrc/mesh_normals.hip through mast3r_slam/normals.py) against their
float32 twin (tests/normals_twin.py), byte for byte, and the lit path of render.render_mesh."""
import numpy as np
import pytest
import torch

import normals_twin as NT
import raster_scenes as RS
from mast3r_slam import normals, render

pytestmark = pytest.mark.gpu


def _degenerate():
    V, F, _ = NT.degenerate()
    return V, F


MESHES = {
    "sheet_17x13": lambda: NT.sheet(17, 13),                 # 221 vertices, 384 faces: less than one workgroup of tail
    "sheet_37x29": lambda: NT.sheet(37, 29),                 # 1073 vertices, 2016 faces: several workgroups, both tails
    "two_sheets": NT.two_sheets,
    "fan": NT.fan,                                           # 4096 faces on one hub: a wave's adds land on one address
    "sphere": lambda: NT.sphere(3),
    "degenerate": _degenerate,
}


def to(dev, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def same_bytes(t, a):
    return t.cpu().numpy().tobytes() == a.tobytes()


# ---- 1. normals --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MESHES))
def test_normals_equal_the_twin_and_do_not_depend_on_the_face_order(dev, name):
    V, F = MESHES[name]()
    if name == "sheet_17x13":
        assert (len(V), len(F)) == (221, 384)
    if name == "sheet_37x29":
        assert (len(V), len(F)) == (1073, 2016)
    want = NT.vertex_normals(V, F)
    v, f = to(dev, V, F)
    got = normals.vertex_normals(v, f)
    assert got.dtype == torch.float32 and got.shape == (len(V), 3) and got.device == v.device
    assert same_bytes(got, want)
    for seed in (1, 2):
        assert same_bytes(normals.vertex_normals(v, to(dev, NT.permuted(F, seed))[0]), want)
    if name == "degenerate":
        zero = NT.degenerate()[2]
        assert not got[torch.from_numpy(zero).to(dev)].any() and torch.isfinite(got).all()


def test_repeat_workspace_reuse_and_out(dev):
    V, F = NT.sheet(37, 29)
    want = NT.vertex_normals(V, F)
    v, f = to(dev, V, F)
    c = torch.zeros((len(V), 3), dtype=torch.uint8, device=dev)
    assert same_bytes(normals.vertex_normals(v, f), want) and same_bytes(normals.vertex_normals(v, f), want)
    ws = torch.full((normals.workspace_bytes(len(V)),), 0xFF, dtype=torch.uint8, device=dev)       # the clear is real
    out = torch.full((len(V), 3), float("nan"), dtype=torch.float32, device=dev)
    got = normals.vertex_normals(v, f, out=out, workspace=ws)
    assert got.data_ptr() == out.data_ptr() and same_bytes(out, want)
    ws.fill_(0xFF)
    assert same_bytes(normals.vertex_normals(v, f, workspace=ws), want)
    assert same_bytes(normals.vertex_normals(v, f, workspace=ws), want)        # and over the sums of the call before
    # the mesh tuple, whole or unpacked, with or without an index behind it
    index = torch.arange(len(V), dtype=torch.int64, device=dev)
    for args in (((v, c, f),), (v, c, f), ((v, c, f, index),), (v, c, f, index)):
        assert same_bytes(normals.vertex_normals(*args), want)
    with pytest.raises(ValueError, match="workspace"):
        normals.vertex_normals(v, f, workspace=ws[:-16])
    with pytest.raises(ValueError):
        normals.vertex_normals(v, f, out=out[:-1])


def test_empty_inputs(dev):
    V, _ = NT.sheet(5, 4)
    v, = to(dev, V)
    none = torch.zeros((0, 3), dtype=torch.int32, device=dev)
    got = normals.vertex_normals(v, none)
    assert got.shape == (20, 3) and not got.any()
    got = normals.vertex_normals(v[:0], none)
    assert got.shape == (0, 3) and got.dtype == torch.float32
    faces_without_vertices = torch.zeros((4, 3), dtype=torch.int32, device=dev)     # every index is outside [0, 0)
    assert normals.vertex_normals(v[:0], faces_without_vertices).shape == (0, 3)
    lit = normals.shade_vertices(v[:0], got, None, light=(0, 0, 1))
    assert lit.shape == (0, 3) and lit.dtype == torch.uint8


# ---- 2. shading ----------------------------------------------------------------------------------------------------------
SHADES = {
    "headlight_one_sided": dict(two_sided=False),
    "headlight_two_sided": dict(two_sided=True),
    "directional": dict(light=(0.3, -0.5, -1.0), two_sided=False),
    "albedo": dict(colors=None, albedo=(180, 200, 90)),
    "normals": dict(mode="normals"),
    "ambient_0": dict(ambient=0.0, two_sided=False),
    "ambient_1": dict(ambient=1.0),
}


@pytest.fixture(scope="module")
def lit_scene():
    """The two-sheet scene with a quarter of its faces flipped (so the one-sided light meets back faces), its normals from
    the twin, and a vertex with a NaN normal, one with a zero normal and one at the eye."""
    sc = RS.general("mixed")
    V, F, C = sc["vertices"].copy(), sc["faces"], sc["colors"]
    eye = sc["view"][:3].copy()
    V[7] = eye                                                                   # l = 0: 0 / 0
    N = NT.vertex_normals(V, F)
    N[3], N[5] = np.nan, 0.0
    return dict(V=V, F=F, C=C, N=N, view=sc["view"], eye=eye)


@pytest.mark.parametrize("name", list(SHADES))
def test_shade_equals_the_twin(dev, lit_scene, name):
    s, kw = lit_scene, dict(SHADES[name])
    twin_kw = dict(kw)
    colors = twin_kw.pop("colors", s["C"])
    if "light" not in kw and kw.get("mode") != "normals":
        twin_kw["eye"] = s["eye"]
    want32 = NT.shade(s["V"], s["N"], colors, **twin_kw)
    want64 = NT.shade(s["V"], s["N"], colors, dtype=np.float64, **twin_kw)
    v, n, c, view = to(dev, s["V"], s["N"], s["C"], s["view"])
    got = normals.shade_vertices(v, n, kw.pop("colors", c), view, **kw)
    assert got.dtype == torch.uint8 and got.shape == v.shape
    assert same_bytes(got, want32)
    diff = np.abs(got.cpu().numpy().astype(np.int32) - want64.astype(np.int32))
    print(f"{name}: {int((diff > 0).sum())} of {diff.size} channels differ from the float64 twin, at most {int(diff.max())}")
    assert diff.max() <= 1
    out = torch.zeros_like(got)
    assert normals.shade_vertices(v, n, SHADES[name].get("colors", c), view, out=out, **kw).data_ptr() == out.data_ptr()
    assert torch.equal(out, got)
    if name == "headlight_one_sided":
        assert (want32 != NT.shade(s["V"], s["N"], colors, eye=s["eye"], two_sided=True)).any()       # back faces are there
    with pytest.raises(ValueError):
        normals.shade_vertices(v, n[:-1], c, view)


# ---- 3. the lit rasteriser path ---------------------------------------------------------------------------------------------
def draw(sc, mesh, view, **kw):
    return render.render_mesh(*mesh, view, sc["K"], sc["size"], return_index=True, **dict(sc["kw"], **kw))


def test_lit_render_is_render_of_the_shaded_colours(dev):
    sc = RS.general("front")
    mesh = to(dev, sc["vertices"], sc["colors"], sc["faces"])
    view, = to(dev, sc["view"])
    plain = draw(sc, mesh, view)
    assert all(torch.equal(a, b) for a, b in zip(plain, draw(sc, mesh, view, shading=None)))
    n = normals.vertex_normals(mesh[0], mesh[2])
    for shading, shade_kw, mode in (("headlight", None, "lambert"), ("headlight", dict(ambient=0.1, two_sided=False), "lambert"),
                                    ("headlight", dict(colors=None, albedo=(250, 250, 250)), "lambert"),
                                    ("headlight", dict(light=(0.0, -1.0, -1.0)), "lambert"), ("normals", None, "normals")):
        kw = dict(dict(colors=mesh[1]), **(shade_kw or {}))
        shaded = normals.shade_vertices(mesh[0], n, kw.pop("colors"), view, mode=mode, **kw)
        want = draw(sc, (mesh[0], shaded, mesh[2]), view)
        for got in (draw(sc, mesh, view, shading=shading, shade_kw=shade_kw), draw(sc, mesh, view, shading=shading, shade_kw=shade_kw, normals=n),
                    render.render_mesh(mesh, view, sc["K"], sc["size"], return_index=True, shading=shading, shade_kw=shade_kw, **sc["kw"])):
            assert all(torch.equal(a, b) for a, b in zip(got, want))
        assert torch.equal(want[1], plain[1]) and torch.equal(want[2], plain[2]) and not torch.equal(want[0], plain[0])
    with pytest.raises(ValueError):
        draw(sc, mesh, view, shading="headlight", shade_kw=dict(mode="normals"))
    with pytest.raises(ValueError):
        draw(sc, mesh, view, shading="headlight", normals=n[:-1])


def test_a_lit_sphere_is_brighter_at_the_centre_than_at_the_limb(dev):
    V, F = NT.sphere(4)
    v, f = to(dev, V, F)
    c = torch.zeros((len(V), 3), dtype=torch.uint8, device=dev)                 # the photographs are not used
    view = render.look_at((0.0, 0.0, -3.0), (0.0, 0.0, 0.0)).to(dev)
    size, K = (96, 96), (120.0, 120.0, 47.5, 47.5)
    rgb, depth = render.render_mesh(v, c, f, view, K, size, cull="back", shading="headlight",
                                    shade_kw=dict(colors=None, albedo=(240, 240, 240), ambient=0.1, two_sided=False))
    rgb, depth = rgb.cpu().numpy().astype(np.int32), depth.cpu().numpy()
    # the silhouette has radius 120 / sqrt(8) = 42.4 pixels; 38.5 pixels from the centre the cosine is about 0.4
    assert np.isfinite(depth[48, 48]) and np.isfinite(depth[48, 86]) and not np.isfinite(depth[2, 2])
    centre, limb = rgb[48, 48], rgb[48, 86]
    print(f"centre {centre.tolist()}, limb {limb.tolist()}")
    assert (centre > 230).all() and (limb < centre - 60).all() and (limb >= 24).all()
    assert (rgb[2, 2] == 0).all()


# ---- 4. graph capture ---------------------------------------------------------------------------------------------------------
def test_graph_replay_follows_the_eye(dev):
    sa, sb = RS.general("front"), RS.general("oblique")                        # the same mesh from two poses
    mesh, size = to(dev, sa["vertices"], sa["colors"], sa["faces"]), sa["size"]
    v = len(sa["vertices"])
    shade_kw = dict(two_sided=False, ambient=0.1)

    def eager(sc):
        view, = to(dev, sc["view"])
        return [t.cpu().numpy() for t in draw(sc, mesh, view, shading="headlight", shade_kw=shade_kw)]

    want_a, want_b = eager(sa), eager(sb)
    assert want_a[0].tobytes() != want_b[0].tobytes()
    pose, = to(dev, sa["view"])
    nrm = torch.empty((v, 3), dtype=torch.float32, device=dev)
    lit = torch.empty((v, 3), dtype=torch.uint8, device=dev)
    nws = torch.empty(normals.workspace_bytes(v), dtype=torch.uint8, device=dev)
    out = (torch.empty((*size, 3), dtype=torch.uint8, device=dev), torch.empty(size, dtype=torch.float32, device=dev),
           torch.empty(size, dtype=torch.int64, device=dev))
    ws = torch.empty(render.mesh_workspace_bytes(v, size), dtype=torch.uint8, device=dev)

    def run():
        normals.vertex_normals(mesh[0], mesh[2], out=nrm, workspace=nws)
        normals.shade_vertices(mesh[0], nrm, mesh[1], pose, out=lit, **shade_kw)
        render.render_mesh(mesh[0], lit, mesh[2], pose, sa["K"], size, return_index=True, out=out, workspace=ws, **sa["kw"])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                            # warm-up outside the capture
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for o in out + (nrm, lit):
        o.zero_()
    nws.fill_(0xFF)                                                            # the replay clears the sums itself
    graph.replay()
    assert same_bytes(nrm, NT.vertex_normals(sa["vertices"], sa["faces"]))
    assert all(o.cpu().numpy().tobytes() == w.tobytes() for o, w in zip(out, want_a))
    pose.copy_(to(dev, sb["view"])[0])                                         # in place: the graph holds the address
    graph.replay()                                                             # over the sums of the replay before
    assert same_bytes(nrm, NT.vertex_normals(sa["vertices"], sa["faces"]))
    assert all(o.cpu().numpy().tobytes() == w.tobytes() for o, w in zip(out, want_b))
