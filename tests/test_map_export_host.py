"""CPU: the map and trajectory writers of mast3r_slam/export.py, the Keyframes getters and the argument checks of
collect_map.  The expected files are built here from the reference's text (slam.py:354-415): PLY vertex properties
`float x y z, uchar red green blue`, TUM `ts tx ty tz qx qy qz qw`, KITTI the first three rows of [sR | t], all %.6f."""
import os

import numpy as np
import pytest
import torch

from mast3r_slam import _ffi, export, mast3r_utils
from mast3r_slam.frame import Frame, Keyframes

PLY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
PROPS = ["property float x", "property float y", "property float z", "property uchar red", "property uchar green",
         "property uchar blue"]


def read_header(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    return raw[:end].decode("ascii").splitlines(), end


def cloud(m, seed=0):
    rng = np.random.default_rng(seed)
    p = (rng.normal(size=(m, 3)) * 10).astype(np.float32)
    if m > 4:
        p[1] = [np.float32(1e-30), -0.0, 3.4e38]
        p[2] = [1 / 3, -2 / 3, 123456.789]
    c = rng.integers(0, 256, size=(m, 3)).astype(np.uint8)
    return p, c


@pytest.mark.parametrize("m", [0, 1, 1000])
@pytest.mark.parametrize("as_tensor", [False, True])
def test_save_ply_binary_round_trip(tmp_path, m, as_tensor):
    p, c = cloud(m)
    path = tmp_path / "map.ply"
    n = export.save_ply(path, torch.from_numpy(p) if as_tensor else p, torch.from_numpy(c) if as_tensor else c)
    assert n == m
    lines, hdr = read_header(path)
    assert lines == ["ply", "format binary_little_endian 1.0", f"element vertex {m}", *PROPS, "end_header"]
    assert os.path.getsize(path) == hdr + 15 * m
    body = np.fromfile(path, dtype=PLY_DTYPE, offset=hdr)
    assert body.shape == (m,)
    back = np.ascontiguousarray(np.stack([body["x"], body["y"], body["z"]], axis=1).reshape(-1, 3))
    assert back.view(np.uint32).tolist() == p.view(np.uint32).tolist()            # bit for bit (-0.0, tiny values)
    assert np.array_equal(np.stack([body["red"], body["green"], body["blue"]], axis=1).reshape(-1, 3), c)


def test_save_ply_ascii_matches_the_reference_format(tmp_path):
    p, c = cloud(50, seed=3)
    path = tmp_path / "map_ascii.ply"
    assert export.save_ply(path, p, c, binary=False) == 50
    want = ["ply", "format ascii 1.0", "element vertex 50", *PROPS, "end_header"]
    want += [f"{a[0]:.6f} {a[1]:.6f} {a[2]:.6f} {b[0]} {b[1]} {b[2]}" for a, b in zip(p, c)]   # slam.py:411-412
    assert open(path).read() == "\n".join(want) + "\n"
    path0 = tmp_path / "empty.ply"
    assert export.save_ply(path0, p[:0], c[:0], binary=False) == 0
    assert open(path0).read().splitlines() == ["ply", "format ascii 1.0", "element vertex 0", *PROPS, "end_header"]


def test_save_ply_rejects_mismatched_lengths(tmp_path):
    p, c = cloud(5)
    with pytest.raises(ValueError):
        export.save_ply(tmp_path / "x.ply", p, c[:4])


def poses_f32():
    rng = np.random.default_rng(11)
    q = rng.normal(size=(4, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    P = np.concatenate([rng.normal(size=(4, 3)) * 3, q, [[1.0], [1.2], [0.37], [2.5]]], axis=1).astype(np.float32)
    P[0, 3:7] = [0, 0, 0, 1]
    return P, [0.0, 0.1, 1234567.891234, 3.5]


def quat_matrix64(q):
    x, y, z, w = [float(v) for v in q]                                  # liegroups/so3.py:174-205
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=np.float64)


@pytest.mark.parametrize("as_tensor", [False, True])
def test_save_trajectory_tum(tmp_path, as_tensor):
    P, ts = poses_f32()
    path = tmp_path / "traj.txt"
    assert export.save_trajectory(path, ts, torch.from_numpy(P) if as_tensor else P, format="tum") == 4
    want = [" ".join(f"{float(v):.6f}" for v in [t, *row[:7]]) for t, row in zip(ts, P)]
    assert open(path).read() == "\n".join(want) + "\n"


def test_save_trajectory_kitti_is_sR_t(tmp_path):
    P, ts = poses_f32()
    path = tmp_path / "traj_kitti.txt"
    assert export.save_trajectory(path, ts, P, format="kitti") == 4
    want = []
    for row in P.astype(np.float64):
        T = np.concatenate([row[7] * quat_matrix64(row[3:7]), row[:3, None]], axis=1)       # [sR | t], 3 x 4
        want.append(" ".join(f"{v:.6f}" for v in T.flatten()))
    assert open(path).read() == "\n".join(want) + "\n"
    second = np.array([float(v) for v in want[1].split()]).reshape(3, 4)
    assert abs(np.linalg.det(second[:, :3]) - 1.2 ** 3) < 1e-4                               # the scale is in the matrix


def test_save_trajectory_errors(tmp_path):
    P, ts = poses_f32()
    with pytest.raises(ValueError):
        export.save_trajectory(tmp_path / "t.txt", ts, P, format="euroc")
    assert not os.path.exists(tmp_path / "t.txt")
    with pytest.raises(ValueError):
        export.save_trajectory(tmp_path / "t.txt", ts[:3], P, format="tum")


def frame(i, n, img, count=1):
    f = Frame(frame_id=i, img=img, T_WC=torch.tensor([[0, 0, 0, 0, 0, 0, 1, 1.0]]))
    f.X_canon, f.C, f.N = torch.zeros(n, 3), torch.ones(n, 1), count
    return f


def test_collect_map_argument_errors():
    ok = torch.zeros(3, 4, 5)
    with pytest.raises(ValueError, match="points"):
        export.collect_map([frame(0, 20, ok), frame(1, 24, torch.zeros(3, 4, 6))])          # mixed point counts
    with pytest.raises(ValueError, match="pixels"):
        export.collect_map([frame(0, 20, torch.zeros(3, 4, 6))])                              # H*W != N
    for bad in (torch.zeros(3, 4, 5, dtype=torch.float64), torch.zeros(4, 5, 3), torch.zeros(3, 4, 5, dtype=torch.uint8),
                torch.zeros(20, 3), torch.zeros(4, 5, 4, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="image"):
            export.collect_map([frame(0, 20, bad)])
    with pytest.raises(ValueError, match="mix"):
        export.collect_map([frame(0, 20, ok), frame(1, 20, torch.zeros(4, 5, 3, dtype=torch.uint8))])
    with pytest.raises(ValueError, match="voxel_size"):
        export.collect_map([frame(0, 20, ok)], voxel_size=0.0)
    with pytest.raises(RuntimeError):                                                         # valid, but on the CPU
        export.collect_map([frame(0, 20, ok)])


def test_collect_map_without_keyframes_is_empty():
    empty = Frame(frame_id=0, img=torch.zeros(3, 4, 5), T_WC=torch.zeros(1, 8))              # no pointmap: skipped
    for kfs in (Keyframes(), [], [empty]):
        p, c, i = export.collect_map(kfs, return_index=True)
        assert p.shape == (0, 3) and p.dtype == torch.float32
        assert c.shape == (0, 3) and c.dtype == torch.uint8
        assert i.shape == (0,) and i.dtype == torch.int64
        assert len(export.collect_map(kfs)) == 2


def test_keyframes_getters():
    kfs = Keyframes()
    assert kfs.get_poses().shape == (1, 8) and kfs.get_poses()[0].tolist() == [0, 0, 0, 0, 0, 0, 1, 1]
    assert kfs.get_points().shape[0] == 0 and kfs.get_confidences().shape[0] == 0
    g = torch.Generator().manual_seed(0)
    for i in range(3):
        f = frame(i, 20, torch.zeros(3, 4, 5), count=i + 1)
        f.T_WC = torch.randn(1, 8, generator=g)
        f.X_canon, f.C = torch.randn(20, 3, generator=g), torch.rand(20, 1, generator=g) * 4
        kfs.append(f)
    assert torch.equal(kfs.get_poses(), torch.cat([f.T_WC for f in kfs._frames])) and kfs.get_poses().shape == (3, 8)
    assert torch.equal(kfs.get_points(), torch.stack([f.X_canon for f in kfs._frames])) and kfs.get_points().shape == (3, 20, 3)
    conf = kfs.get_confidences()
    assert conf.shape == (3, 20, 1)
    for i, f in enumerate(kfs._frames):
        assert torch.equal(conf[i], f.C / (i + 1))                          # the AVERAGE confidence (frame.py:251)


def test_symbols_are_declared_and_re_exported():
    names = _ffi.declared_symbols()
    for n in ("m3_map_export_ws_bytes", "m3_map_export_count", "m3_map_export_scatter", "m3_map_voxel_table_slots",
              "m3_map_voxel_ws_bytes", "m3_map_voxel_count", "m3_map_voxel_scatter"):
        assert n in names
    for n in ("collect_map", "save_ply", "save_trajectory"):
        assert n in mast3r_utils.__all__ and getattr(mast3r_utils, n) is getattr(export, n)


def test_entry_points_validate_before_any_device_call():
    L = _ffi.lib()
    assert L.m3_abi_version() == 4000                                        # symbols were added, nothing changed
    assert L.m3_map_export_ws_bytes(256, 512 * 512) == (4 + 256 * 256) * 4 and L.m3_map_export_ws_bytes(1, 3) == 32
    assert L.m3_map_export_ws_bytes(0, 4) == 0 and L.m3_map_export_ws_bytes(4, 0) == 0
    assert L.m3_map_export_ws_bytes(1 << 16, 1 << 16) == 0                  # 2^32 points: beyond the int32 offsets
    assert L.m3_map_voxel_table_slots(1000) == 2048 and L.m3_map_voxel_table_slots(0) == 0
    assert L.m3_map_voxel_ws_bytes(1000) == (4 + 4) * 4 + 1000 * 4 + 2 * 2048 * 8
    assert L.m3_map_export_count(None, None, None, None, 1, 4, 1, 1.5, None, 64, None) == -1
    assert L.m3_map_export_scatter(None, None, None, None, None, 1, 4, 1, 1.5, 0, None, 64, 1, None, None, None, None,
                                   None) == -1
    assert L.m3_map_voxel_count(None, None, 4, 0.1, None, 1 << 20, None) == -1
    assert L.m3_map_voxel_scatter(None, None, None, 4, None, 1 << 20, 1, None, None, None, None) == -1
