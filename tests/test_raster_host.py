"""No GPU: the rasteriser's twin (tests/raster_twin.py) against its own fp32 emulation on every scene the GPU tests use,
the coverage rule's exactly-once property, and the argument checks of render_mesh, SLAM.render_view and ViewRecorder
that run before the device is touched."""
import numpy as np
import pytest
import torch

import raster_scenes as RS
import raster_twin as RW
from mast3r_slam import mast3r_utils, render
from mast3r_slam.slam import SLAM


def twin_and_emulation(sc, **kw):
    args = (sc["vertices"], sc["colors"], sc["faces"], sc["view"], sc["K"], sc["size"])
    kw = dict(sc["kw"], **kw)
    return RW.raster_twin(*args, **kw), RW.fp32_emulation(*args, **kw)


@pytest.mark.parametrize("label,sc", list(RS.twin_scenes()), ids=[l for l, _ in RS.twin_scenes()])
def test_fp32_emulation_agrees_with_the_float64_twin(label, sc):
    for cull in ("none", "back"):
        tw, em = twin_and_emulation(sc, cull=cull)
        share = RW.check_against_twin(tw, *em, f"{label} cull={cull}")       # prints the contested share; asserts the cap
        assert share <= RW.MAX_CONTESTED and tw["covered"].any()


@pytest.mark.parametrize("size,offset,shared", RS.EXACT)
def test_exact_scenes_are_exact_in_fp32(size, offset, shared):
    sc = RS.exact(size, offset, 3, shared)
    a = RW.vertex_stage(sc["vertices"], sc["view"], sc["K"], 0.5, np.inf)
    b = RW.vertex_stage(sc["vertices"], sc["view"], sc["K"], 0.5, np.inf, np.float32)
    assert all(np.array_equal(a[k], b[k]) for k in ("sx", "sy", "z", "ok", "guard"))
    tw, em = twin_and_emulation(sc)
    # same snapped vertices: the integer coverage is the same, and the winners differ only where depths tie within fp32
    assert np.array_equal(tw["covered"], em[2] >= 0) and tw["covered"].all()
    free = ~tw["contested"]
    assert np.array_equal(tw["index"][free], em[2][free])
    won = em[2]
    assert ((won < sc["originals"]) | (won == len(sc["faces"]) - 1)).all()     # a repeated face never beats its first copy
    print(f"{size} offset {offset}: {int((tw['contested'] & tw['covered']).sum())} of {tw['covered'].sum()} pixels on an edge or tied")


def test_planar_sheet_and_its_subdivision_cover_the_same_pixels():
    sc = RS.planar_sheet()
    sub = RS.subdivided(sc)
    assert RS.box_pixels(sc).min() > 64 and RS.box_pixels(sub).max() <= 64    # the two sides of the walk threshold
    ta, a = twin_and_emulation(sc)
    tb, b = twin_and_emulation(sub)
    assert RW.check_same_surface(ta, a, tb, b, "fp32 emulation") > 1000
    assert RW.check_same_surface(ta, (ta["rgb"], ta["depth"], ta["index"]), tb, (tb["rgb"], tb["depth"], tb["index"]), "float64") > 1000


def aligned_sheet(winding):
    nx, ny = 9, 7
    sx = np.array([i * 8 * RW.S for j in range(ny) for i in range(nx)], dtype=np.int64)
    sy = np.array([j * 8 * RW.S for j in range(ny) for i in range(nx)], dtype=np.int64)
    _, F = RS.sheet(nx, ny, lambda X, Y: X, 0, 1, 0, 1)
    if winding == "flipped":
        F = F[:, [0, 2, 1]]
    elif winding == "mixed":
        F = np.where((np.arange(len(F)) % 2 == 0)[:, None], F, F[:, [0, 2, 1]])
    ok = np.ones(nx * ny, dtype=bool)
    return dict(sx=sx, sy=sy, ok=ok, guard=ok, z=np.ones(nx * ny)), F


@pytest.mark.parametrize("winding", ["ccw", "flipped", "mixed"])
def test_a_pixel_aligned_sheet_is_covered_exactly_once(winding):
    vs, F = aligned_sheet(winding)
    Hv, Wv = 56, 72
    Y, X = np.meshgrid(np.arange(Hv, dtype=np.int64) * RW.S, np.arange(Wv, dtype=np.int64) * RW.S, indexing="ij")
    count = np.zeros((Hv, Wv), dtype=np.int64)
    for face in F:
        rows, _ = RW._oriented(vs, face, 0)
        inside = np.ones((Hv, Wv), dtype=bool)
        for E, top_left, _ in RW._edges(vs, rows, X, Y):
            inside &= (E > 0) | ((E == 0) & top_left)
        count += inside
    # every vertex on a pixel centre, every edge through pixel centres: rows 0 ... 47 and columns 0 ... 63, once each
    assert (count[:48, :64] == 1).all() and count[48:].sum() == 0 and count[:, 64:].sum() == 0


def mesh(v=4, f=2):
    return (torch.zeros((v, 3), dtype=torch.float32), torch.zeros((v, 3), dtype=torch.uint8), torch.zeros((f, 3), dtype=torch.int32))


@pytest.mark.parametrize("kw", [dict(size=(0, 5)), dict(size=(4, 5, 6)), dict(cull="front"), dict(background=(0, 0, 256)),
                                dict(background=(0, 0)), dict(near=2.0, far=1.0), dict(near=-1.0), dict(near=float("nan")),
                                dict(K=(0.0, 1.0, 2.0, 2.0))])
def test_render_mesh_rejects_bad_arguments(kw):
    kw = dict(dict(size=(4, 5), K=None), **kw)
    with pytest.raises(ValueError):
        render.render_mesh(*mesh(), torch.zeros(8), **kw)


def test_render_mesh_rejects_bad_meshes():
    pose = torch.zeros(8)
    v, c, f = mesh()
    with pytest.raises(ValueError, match="rows"):
        render.render_mesh(v, c[:3], f, pose, None, (4, 5))
    with pytest.raises(ValueError, match="faces"):
        render.render_mesh(v, c, f.to(torch.int64), pose, None, (4, 5))
    with pytest.raises(ValueError, match="vertices"):
        render.render_mesh(v.to(torch.float64), c, f, pose, None, (4, 5))
    with pytest.raises(ValueError, match="faces"):
        render.render_mesh((v, c, f.reshape(-1)), pose, None, (4, 5))         # the tuple form reaches the same checks
    with pytest.raises(ValueError):
        render.render_mesh((v, c), pose, None, (4, 5))
    with pytest.raises(RuntimeError, match="no CPU path"):
        render.render_mesh((v, c, f), pose, None, (4, 5))                      # everything valid, but on the CPU
    assert mast3r_utils.render_mesh is render.render_mesh and mast3r_utils.mesh_workspace_bytes is render.mesh_workspace_bytes
    assert "render_mesh" in render.__all__ and "mesh_workspace_bytes" in render.__all__


def test_workspace_bytes_and_launch_counts():
    from mast3r_slam import _ffi
    L = _ffi.lib()
    assert render.mesh_workspace_bytes(0, (3, 5)) == 128 and render.mesh_workspace_bytes(7, (3, 5)) == 7 * 16 + 128
    assert render.mesh_workspace_bytes(1, (1, 1)) == 32                        # 16 + 8, rounded up to 16
    assert L.m3_raster_launches(0) == 2 and L.m3_raster_launches(1) == L.m3_raster_launches(2 ** 31 - 1) == 4
    for v, size in ((2 ** 31, (3, 5)), (-1, (3, 5)), (1, (0, 5)), (1, (3, 16385))):
        with pytest.raises(ValueError):
            render.mesh_workspace_bytes(v, size)


def test_surface_keyword_is_checked(tmp_path):
    slam = object.__new__(SLAM)                                               # the check comes before any state is read
    with pytest.raises(ValueError, match="surface"):
        SLAM.render_view(slam, surface="bogus")
    with pytest.raises(ValueError, match="surface"):
        SLAM.save_view(slam, tmp_path / "x.png", surface="bogus")
    with pytest.raises(ValueError, match="too costly"):
        render.ViewRecorder(tmp_path, surface="fused")
    with pytest.raises(ValueError, match="surface"):
        render.ViewRecorder(tmp_path, surface="bogus")
    assert render.ViewRecorder(tmp_path, surface="mesh", mesh_kw=dict(stride=2)).surface == "mesh"
    assert render.ViewRecorder(tmp_path).surface == "points"
