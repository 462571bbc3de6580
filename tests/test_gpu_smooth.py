"""GPU: mesh_topology and smooth_mesh (csrc/mesh_smooth.hip) against the numpy twin of the header's rule
(tests/smooth_twin.py), as bytes: no tolerance anywhere.  The scenes cover more than one workgroup with a last one that
is not full (the grid), a row longer than a wave (the fan), every odd face the rule names and vertices that are not
finite (odd), sums that need float64 (offset), a closed surface (icosphere) and exact arithmetic (lattice)."""
import numpy as np
import pytest
import torch

import smooth_twin as ST
from mast3r_slam import smooth

pytestmark = pytest.mark.gpu
SCENES = sorted(ST.SCENES)
COUNTS = ("edges", "boundary_edges", "nonmanifold_edges", "invalid_faces")


@pytest.fixture(scope="module")
def scenes():
    return {name: make() for name, make in ST.SCENES.items()}


def upload(mesh, dev):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in mesh)


def raw(t):
    return t.cpu().numpy().tobytes()


def pin_mask(V):
    return np.random.default_rng(V).random(V) < 0.2


def check_topology(got, want):
    assert [getattr(got, n) for n in COUNTS] == [want[n] for n in COUNTS]
    assert got.degree.dtype == torch.int32 and raw(got.degree) == want["degree"].tobytes()
    assert got.boundary.dtype == torch.bool and raw(got.boundary) == want["boundary"].tobytes()
    if got.edge_rows is not None:
        assert got.edge_rows.dtype == got.edge_faces.dtype == torch.int32
        assert tuple(got.edge_rows.shape) == want["edge_rows"].shape and raw(got.edge_rows) == want["edge_rows"].tobytes()
        assert tuple(got.edge_faces.shape) == want["edge_faces"].shape and raw(got.edge_faces) == want["edge_faces"].tobytes()


@pytest.mark.parametrize("scene", SCENES)
def test_topology_equals_the_twin(dev, scenes, scene):
    mesh = scenes[scene]
    v, c, f = upload(mesh, dev)
    V = v.shape[0]
    want = ST.topology(mesh[2], V)
    before = f.clone()
    for _ in range(2):                                                          # every call twice
        check_topology(smooth.mesh_topology(f, V, return_edges=True), want)
    plain = smooth.mesh_topology(f, V)
    assert plain.edge_rows is None and plain.edge_faces is None
    check_topology(plain, want)
    assert torch.equal(f, before)
    ws = torch.empty(smooth.workspace_bytes(V, f.shape[0]) + 64, dtype=torch.uint8, device=dev).fill_(0xa5)
    check_topology(smooth.mesh_topology(f, V, return_edges=True, workspace=ws), want)       # contents ignored on entry
    other = torch.from_numpy(ST.shuffled(mesh[2], 1234)).to(dev)                # the canonical rows: any face order
    check_topology(smooth.mesh_topology(other, V, return_edges=True), want)


@pytest.mark.parametrize("scene", SCENES)
def test_smooth_equals_the_twin(dev, scenes, scene):
    mesh = scenes[scene]
    v, c, f = upload(mesh, dev)
    V = v.shape[0]
    before = [t.clone() for t in (v, c, f)]
    other = torch.from_numpy(ST.shuffled(mesh[2], 4321)).to(dev)
    pin = pin_mask(V)
    pin_dev = torch.from_numpy(pin).to(dev)
    cases = [dict(method=m, iterations=it, fix_boundary=fb) for m in ("taubin", "laplacian") for it in (0, 1, 3) for fb in (False, True)]
    cases += [dict(method="taubin", iterations=3, pinned=pin), dict(method="laplacian", iterations=1, fix_boundary=True, pinned=pin),
              dict(method="laplacian", iterations=2, lam=1.0), dict(method="taubin", iterations=2, lam=0.33, mu=-0.34)]
    for kw in cases:
        want = ST.smooth(mesh[0], mesh[2], **kw).tobytes()
        if "pinned" in kw:
            kw = dict(kw, pinned=pin_dev)
        got = smooth.smooth_mesh(v, c, f, **kw)
        assert got[0].dtype == torch.float32 and tuple(got[0].shape) == (V, 3) and raw(got[0]) == want, kw
        assert got[1] is c and got[2] is f and got[0].data_ptr() != v.data_ptr()
        assert raw(smooth.smooth_mesh(v, c, f, **kw)[0]) == want, kw              # twice
        whole = smooth.smooth_mesh((v, c, f), **kw)                               # whole or unpacked
        assert raw(whole[0]) == want and whole[1] is c and whole[2] is f, kw
        assert raw(smooth.smooth_mesh(v, c, other, **kw)[0]) == want, kw          # any order of the face rows
    assert all(raw(a) == raw(b) for a, b in zip((v, c, f), before))             # the inputs are as they were
    assert raw(pin_dev) == pin.tobytes()


def test_defaults_are_ten_taubin_iterations(dev, scenes):
    mesh = scenes["icosphere"]
    got = smooth.smooth_mesh(upload(mesh, dev))
    assert raw(got[0]) == ST.smooth(mesh[0], mesh[2], iterations=10, method="taubin", lam=0.5, mu=-0.53).tobytes()


def test_integer_lattice_needs_no_twin(dev, scenes):
    """Every sum and every mean is exact on the lattice: with the rim pinned nothing moves, whatever the weights."""
    mesh = scenes["lattice"]
    v, c, f = upload(mesh, dev)
    rim = torch.from_numpy(ST.grid_rim(9, 9)).to(dev)
    for it in (1, 4, 10):
        assert raw(smooth.smooth_mesh(v, c, f, iterations=it, method="taubin", fix_boundary=True)[0]) == mesh[0].tobytes()
    assert raw(smooth.smooth_mesh(v, c, f, iterations=5, method="taubin", pinned=rim)[0]) == mesh[0].tobytes()
    one = smooth.smooth_mesh(v, c, f, iterations=1, method="laplacian")[0]
    assert int((~rim).sum()) == 49 and raw(one[~rim]) == mesh[0][~ST.grid_rim(9, 9)].tobytes() and not torch.equal(one[rim], v[rim])


def test_vertices_that_are_not_finite(dev, scenes):
    mesh = scenes["odd"]
    v, c, f = upload(mesh, dev)
    got = smooth.smooth_mesh(v, c, f, iterations=3)[0].cpu().numpy()
    want = ST.smooth(mesh[0], mesh[2], iterations=3)
    for r in (ST.ODD_NAN, ST.ODD_INF):
        assert got[r].tobytes() == mesh[0][r].tobytes()                         # bit for bit
    off, nbr = ST.adjacency(mesh[2], len(mesh[0]))
    around = np.concatenate([nbr[off[r]:off[r + 1]] for r in (ST.ODD_NAN, ST.ODD_INF)])
    assert len(around) == 12 and np.isfinite(got[around]).all() and got[around].tobytes() == want[around].tobytes()
    assert (got[around] != mesh[0][around]).any(axis=1).all()                   # they moved, on their finite neighbours


def test_empty_and_faceless_meshes(dev):
    e = (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.uint8, device=dev),
         torch.empty((0, 3), dtype=torch.int32, device=dev))
    out = smooth.smooth_mesh(e)
    assert tuple(out[0].shape) == (0, 3) and out[0].dtype == torch.float32 and out[1] is e[1] and out[2] is e[2]
    top = smooth.mesh_topology(e[2], 0, return_edges=True)
    assert top[:4] == (0, 0, 0, 0) and tuple(top.degree.shape) == (0,) and tuple(top.boundary.shape) == (0,)
    assert tuple(top.edge_rows.shape) == (0, 2) and tuple(top.edge_faces.shape) == (0,)
    v = torch.from_numpy(np.random.default_rng(3).normal(size=(300, 3)).astype(np.float32)).to(dev)
    c = torch.zeros((300, 3), dtype=torch.uint8, device=dev)
    for kw in (dict(), dict(method="laplacian", iterations=1, fix_boundary=True), dict(iterations=0)):
        assert raw(smooth.smooth_mesh(v, c, e[2], **kw)[0]) == raw(v)           # no edge: nothing moves
    top = smooth.mesh_topology(e[2], 300, return_edges=True)
    assert top[:4] == (0, 0, 0, 0) and not bool(top.degree.any()) and not bool(top.boundary.any()) and top.edge_rows.shape[0] == 0
    # faces that hold no edge at all
    f = torch.tensor([[4, 4, 4], [7, 7, 7]], dtype=torch.int32, device=dev)
    assert raw(smooth.smooth_mesh(v, c, f)[0]) == raw(v) and smooth.mesh_topology(f, 300).edges == 0


def test_rows_out_of_range(dev, scenes):
    mesh = scenes["lattice"]
    V = len(mesh[0])
    bad = np.concatenate([mesh[2], [[0, 1, V], [-1, 2, 3], [2 ** 31 - 1, 0, 1]]]).astype(np.int32)
    v, c, f = upload((mesh[0], mesh[1], bad), dev)
    with pytest.raises(ValueError, match="3 faces name a vertex row outside"):
        smooth.mesh_topology(f, V)
    got = smooth.smooth_mesh(v, c, f, iterations=2, method="laplacian")
    assert raw(got[0]) == ST.smooth(mesh[0], bad, iterations=2, method="laplacian").tobytes()
    assert raw(got[0]) == ST.smooth(mesh[0], mesh[2], iterations=2, method="laplacian").tobytes()     # the faces are ignored


def test_cpu_tensors_raise(dev, scenes):
    v, c, f = (torch.from_numpy(a) for a in scenes["lattice"])
    with pytest.raises(RuntimeError, match="ROCm device"):
        smooth.smooth_mesh(v, c, f)
    with pytest.raises(RuntimeError, match="ROCm device"):
        smooth.mesh_topology(f, len(v))
    d = upload(scenes["lattice"], dev)
    with pytest.raises(ValueError):
        smooth.smooth_mesh(d, pinned=torch.zeros(len(v), dtype=torch.bool))     # a mask on the other device
    with pytest.raises(ValueError):
        smooth.smooth_mesh(d, pinned=torch.zeros(len(v) + 1, dtype=torch.bool, device=dev))
    with pytest.raises(ValueError):
        smooth.smooth_mesh(d, workspace=torch.empty(64, dtype=torch.uint8, device=dev))


def test_graph_replay_gives_the_eager_bytes(dev, scenes):
    mesh = scenes["grid"]
    v, c, f = upload(mesh, dev)
    V = v.shape[0]
    ws = torch.empty(smooth.workspace_bytes(V, f.shape[0]), dtype=torch.uint8, device=dev)
    kw = dict(iterations=3, fix_boundary=True, workspace=ws)
    eager = smooth.smooth_mesh(v, c, f, **kw)[0].clone()
    assert raw(eager) == ST.smooth(mesh[0], mesh[2], iterations=3, fix_boundary=True).tobytes()
    moved = ST.jittered_grid(seed=77)[0]                                        # the same grid, other positions
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                               # warm-up outside the capture
        smooth.smooth_mesh(v, c, f, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                               # one stream: a serial chain of launches
        out = smooth.smooth_mesh(v, c, f, **kw)[0]
    ws.zero_()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert raw(out) == raw(eager)
    v.copy_(torch.from_numpy(moved))                                            # the vertex contents are overwritten
    ws.fill_(0x5a)
    graph.replay()
    torch.cuda.synchronize()
    assert raw(out) == ST.smooth(moved, mesh[2], iterations=3, fix_boundary=True).tobytes()
    assert raw(out) == raw(smooth.smooth_mesh(v, c, f, iterations=3, fix_boundary=True)[0])
