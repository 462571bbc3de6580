"""Host: what tests/test_gpu_shared_tables.py relies on - the numpy mix64 and the inputs that put several keys on the last
slot of a 1024-slot table - and the shared argument handling of the mesh wrappers (mast3r_slam/_mesh_args.py) through
every wrapper: the same error, in the same words, whichever pass is called."""
import re

import numpy as np
import pytest
import torch

import cloud_twin as CT
import simplify_twin as SV
import table_scenes as TS
from mast3r_slam import _mesh_args, cloud, components, normals, register, simplify, smooth


def test_mix64_is_the_splitmix64_finaliser():
    # the first outputs of splitmix64 seeded with 0: its state advances by the golden gamma, then this finaliser
    gamma = 0x9e3779b97f4a7c15
    state = [(gamma * (i + 1)) & (2 ** 64 - 1) for i in range(3)]
    assert [int(x) for x in TS.mix64(np.array(state, dtype=np.uint64))] == [0xe220a8397b1dcdaf, 0x6e789e6aa1b965f4, 0x06c45d188009454f]


def test_keys_on_the_last_slot_exist_at_these_sizes():
    assert len(TS.hot_edges(600)) == 145
    assert len(TS.hot_cells(-8, 8)) == 7
    assert (TS.home(TS.edge_keys(*TS.hot_edges(600).T)) == 1023).all() and (TS.home(TS.cell_keys(TS.hot_cells())) == 1023).all()


def test_the_scenes_fill_a_table_of_1024_slots_past_its_end():
    v, c, f = TS.smooth_mesh()
    assert v.shape == (600, 3) and len(f) <= 170 and 6 * len(f) <= TS.S
    first = TS.edge_keys(f[:, 0], f[:, 1])
    assert (TS.home(first) == TS.S - 1).sum() >= 4 and len(TS.last_slot_keys(first)) >= 4
    assert ((f >= 0) & (f < 600)).all() and (f[:, 0] != f[:, 1]).all()
    p = TS.cloud_points()
    assert len(p) <= 512 and len(TS.last_slot_keys(TS.cell_keys(CT.cells(p, TS.CLOUD_RADIUS)))) == 7
    assert len(TS.cloud_queries()) <= 512
    sv = TS.simplify_mesh()
    cell, _, ok = SV.cells_of(sv[0], 1.0)
    assert len(sv[0]) <= 512 and ok.all() and len(TS.last_slot_keys(TS.cell_keys(cell))) == 7
    vp = TS.voxel_cloud()[0]
    assert len(vp) <= 512 and len(TS.last_slot_keys(TS.cell_keys(np.floor(vp / np.float32(1.0))))) == 7


# ---- the argument module, through every wrapper --------------------------------------------------------------------------
def mesh(V=6):
    return torch.zeros((V, 3)), torch.zeros((V, 3), dtype=torch.uint8), torch.tensor([[0, 1, 2]], dtype=torch.int32)


WRAPPERS = {"filter_components": components.filter_components,
            "simplify_mesh": lambda *a: simplify.simplify_mesh(*a, voxel_size=1.0),
            "simplify_counts": lambda *a: simplify.simplify_counts(*a, voxel_size=1.0),
            "smooth_mesh": smooth.smooth_mesh}
WHOLE = "a mesh is (vertices, colors, faces[, index]), passed whole or unpacked"


def raises(kind, text, call, *args):
    with pytest.raises(kind, match=re.escape(text)):
        call(*args)


@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_mesh_wrappers_reject_the_same_arguments_in_the_same_words(name):
    call = WRAPPERS[name]
    v, c, f = mesh()
    raises(ValueError, WHOLE, call, (v, c, f), c, f)
    raises(ValueError, WHOLE, call, (v, c))
    raises(ValueError, "vertices must be a torch.float32 [n,3] tensor, got torch.float64 (6, 3)", call, v.double(), c, f)
    raises(ValueError, "colors must be a torch.uint8 [n,3] tensor, got torch.float32 (6, 3)", call, v, v, f)
    raises(ValueError, "faces must be a torch.int32 [n,3] tensor, got torch.int64 (1, 3)", call, v, c, f.long())
    raises(ValueError, "faces must be a torch.int32 [n,3] tensor, got torch.int32 (3,)", call, v, c, f.reshape(-1))
    raises(ValueError, "faces must be a torch.int32 [n,3] tensor, got NoneType", call, v, c, None)
    raises(ValueError, "vertices has 6 rows, colors 5", call, v, c[:-1], f)
    raises(RuntimeError, "ROCm device", call, v, c, f)                          # well-formed, but on the host
    raises(RuntimeError, "ROCm device", call, (v, c, f))


def test_faces_only_wrappers_and_normals():
    v, c, f = mesh()
    for call in (lambda x: components.mesh_components(x, 6), lambda x: smooth.mesh_topology(x, 6)):
        raises(ValueError, "faces must be a torch.int32 [n,3] tensor, got torch.int64 (1, 3)", call, f.long())
        raises(ValueError, "faces must be a torch.int32 [n,3] tensor, got list", call, [[0, 1, 2]])
        raises(RuntimeError, "ROCm device", call, f)
    raises(ValueError, WHOLE, normals.vertex_normals, (v, c))
    raises(ValueError, WHOLE, normals.vertex_normals, (v, c, f), f)
    raises(ValueError, WHOLE, normals.vertex_normals, v, c, None)               # colours, and no faces behind them
    raises(ValueError, "faces must be a torch.int32 [n,3] tensor, got torch.int64 (1, 3)", normals.vertex_normals, v, f.long())
    raises(RuntimeError, "ROCm device", normals.vertex_normals, (v, c, f))


def test_two_faults_are_reported_in_each_wrapper_s_own_order():
    """filter_components compares the row counts before it looks at the faces; the others look at all three shapes first;
    mesh_topology looks at the faces before n_vertices."""
    v, c, f = mesh()
    raises(ValueError, "vertices has 6 rows, colors 5", components.filter_components, v, c[:-1], f.long())
    for name in ("simplify_mesh", "simplify_counts", "smooth_mesh"):
        raises(ValueError, "faces must be a torch.int32 [n,3] tensor, got torch.int64 (1, 3)", WRAPPERS[name], v, c[:-1], f.long())
    raises(ValueError, "faces must be a torch.int32 [n,3] tensor, got torch.int64 (1, 3)", smooth.mesh_topology, f.long(), -1)
    raises(ValueError, "n_vertices must lie in 0 ... 2^31 - 1, got -1", smooth.mesh_topology, f, -1)


def test_invalid_faces_and_the_empty_result():
    _mesh_args.raise_invalid_faces(0, 5)
    raises(ValueError, "3 faces name a vertex row outside [0, 5)", _mesh_args.raise_invalid_faces, 3, 5)
    plain, indexed = _mesh_args.empty_mesh_with_index("cpu", False), _mesh_args.empty_mesh_with_index("cpu", True)
    assert [(tuple(t.shape), t.dtype) for t in plain] == [((0, 3), torch.float32), ((0, 3), torch.uint8), ((0, 3), torch.int32)]
    assert len(indexed) == 5 and all(tuple(t.shape) == (0,) and t.dtype == torch.int64 for t in indexed[3:])
    assert _mesh_args.unpack_mesh((1, 2, 3, 4)) == (1, 2, 3) and _mesh_args.unpack_mesh(1, 2, 3) == (1, 2, 3)


def test_take_workspace_words():
    """The workspace is looked at before its device: a host tensor fails the device check of every wrapper alike."""
    for owner in ("the mesh lives", "the cloud lives", "the clouds live"):
        raises(RuntimeError, "ROCm device", _mesh_args.take_workspace, torch.zeros(64, dtype=torch.uint8), 64, torch.device("cpu"), owner)
    for call in (lambda: cloud._workspace(torch.zeros(64, dtype=torch.uint8), 1, torch.device("cpu")),
                 lambda: register._workspace(torch.zeros(64, dtype=torch.uint8), 1, 1, 1, torch.device("cpu"))):
        raises(RuntimeError, "ROCm device", call)
