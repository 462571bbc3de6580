"""CPU: the multi-view consistency rule (tests/consistency_twin.py) against its own fp32 emulation on every scene the GPU
tests use, a hand-made case whose counts are written out, the host checks of mast3r_slam/consistency.py that need no
device, and the exported symbols."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import consistency_twin as CT
from mast3r_slam import _ffi, consistency, mast3r_utils
from mast3r_slam.frame import Frame


def scenes():
    for K, H, W, seed in CT.SHARED:
        sc = CT.shared_scene(K, H, W, seed)
        for label, nbr, _ in CT.tables_of(sc):
            yield f"shared {K}x{H}x{W} {label}", sc, CT.shared_pinhole(H, W), nbr, {}
    sc = CT.shared_scene(5, 33, 65, 15, grid_centres=True)
    yield "grid centres 5x33x65 nearest3", sc, CT.shared_pinhole(33, 65), CT.nearest(sc["T"], 3), {}
    sc = CT.shared_scene(1, 33, 65, 14)
    yield "single 1x33x65", sc, CT.shared_pinhole(33, 65), CT.all_others(1), {}
    for layout in ("f32", "u8"):
        sc, pin, nbr = CT.exact_scene(5, layout)
        yield f"exact {layout}", sc, pin, nbr, dict(z_min=CT.EXACT_ZMIN, depth_rtol=CT.EXACT_RTOL)


def test_emulation_equals_the_twin_on_uncontested_sources():
    for label, sc, pin, nbr, kw in scenes():
        for thr in (1.5, None):
            tw = CT.twin(sc, pin, nbr, thr=thr, **kw)
            s, c, conf = CT.fp32_emulation(sc, pin, nbr, thr=thr, **kw)
            share = CT.contested_share(tw)
            free = tw["pairs"] == 0
            print(f"{label} thr={thr}: {int(tw['cand'].sum())} candidates, contested {100 * share:.2f} %, "
                  f"{int((s != tw['support']).sum() + (c != tw['conflict']).sum())} count differences on contested sources")
            # the exact scene sits on the boundaries on purpose: it is compared on every source instead
            assert share <= CT.MAX_CONTESTED or label.startswith("exact")
            assert np.array_equal(s[free], tw["support"][free]) and np.array_equal(c[free], tw["conflict"][free])
            assert conf[free].tobytes() == tw["conf"][free].tobytes()
            if label.startswith("exact"):                                     # every operation is exact: no source differs
                assert np.array_equal(s, tw["support"]) and np.array_equal(c, tw["conflict"])
                assert conf.tobytes() == tw["conf"].tobytes()


def test_shared_scenes_exercise_every_outcome():
    for K, H, W, seed in CT.SHARED:
        sc = CT.shared_scene(K, H, W, seed)
        tw = CT.twin(sc, CT.shared_pinhole(H, W), CT.all_others(K))
        assert set(np.unique(tw["support"][tw["cand"]])) == set(range(K))          # every support value 0 ... K - 1
        assert tw["conflict"].max() >= 2 and 0 < tw["kept"].sum() < tw["cand"].sum() < K * H * W


def test_exact_scene_contains_its_cases():
    sc, pin, nbr = CT.exact_scene(5)
    cases = CT.exact_scene_cases(sc, pin, nbr)
    print(cases)
    assert cases["boundary"] > 50 and cases["ulp_miss"] == 2 and cases["half"] > 100 and cases["behind"] > 100
    assert cases["outside"] > 20
    tw = CT.twin(sc, pin, nbr, z_min=CT.EXACT_ZMIN, depth_rtol=CT.EXACT_RTOL, min_views=1, max_conflicts=0)
    (m_up, (d_up, z_up)), (m_dn, (d_dn, z_dn)) = sorted(sc["ulp"].items())
    assert z_up > d_up and z_dn < d_dn
    assert tw["cand"][0, m_up] and tw["support"][0, m_up] == 0 and tw["conflict"][0, m_up] == 0    # one ulp behind: occluded
    assert tw["cand"][0, m_dn] and tw["support"][0, m_dn] == 0 and tw["conflict"][0, m_dn] == 1    # one ulp in front: seen through
    # the same pixels one ulp back are boundary agreements
    X = sc["X"].copy()
    X[0, m_up] = X[0, m_up] / np.float32(z_up * 2) * np.float32(2 * d_up * 33 / 32)
    X[0, m_dn] = X[0, m_dn] / np.float32(z_dn * 2) * np.float32(2 * d_dn * 31 / 32)
    tw = CT.twin(dict(sc, X=X), pin, nbr, z_min=CT.EXACT_ZMIN, depth_rtol=CT.EXACT_RTOL)
    assert tw["support"][0, m_up] == 1 and tw["support"][0, m_dn] == 1


def test_hand_made_case():
    sc, pin, support, conflict = CT.hand_case()
    nbr = CT.all_others(3)
    tw = CT.twin(sc, pin, nbr)
    assert np.array_equal(tw["support"], support) and np.array_equal(tw["conflict"], conflict)
    assert tw["pairs"].sum() == 0
    s, c, conf = CT.fp32_emulation(sc, pin, nbr, min_views=1, max_conflicts=1)
    assert np.array_equal(s, support) and np.array_equal(c, conflict)
    kept = np.array([[1, 1, 0, 0], [1, 1, 1, 0], [1, 0, 1, 0]], dtype=bool)
    assert np.array_equal(conf, np.where(kept, sc["C"], -np.inf).astype(np.float32))
    assert np.array_equal(CT.twin(sc, pin, nbr, min_views=1, max_conflicts=0)["kept"],
                          np.array([[1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0]], dtype=bool))
    assert np.array_equal(CT.twin(sc, pin, nbr, min_views=0, max_conflicts=None)["kept"], tw["cand"])
    assert not tw["cand"][2, 3] and tw["cand"].sum() == 11


def test_neighbour_tables():
    assert CT.all_others(4).tolist() == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]]
    assert consistency._all_others(4, "cpu").tolist() == CT.all_others(4).tolist()
    assert consistency._all_others(1, "cpu").shape == (1, 0)
    sc = CT.shared_scene(5, 33, 65, 15, grid_centres=True)
    T = torch.from_numpy(sc["T"])
    for v in (0, 1, 3, 4, 9):
        got = consistency.nearest_neighbours(T, v)
        assert got.dtype == torch.int32 and np.array_equal(got.numpy(), CT.nearest(sc["T"], v))
    assert consistency.nearest_neighbours(T, 9).shape == (5, 4)


def frame(k, h, w, n=None):
    f = Frame(frame_id=k, img=torch.zeros(3, h, w), T_WC=torch.tensor([[0, 0, 0, 0, 0, 0, 1, 1.0]]))
    n = h * w if n is None else n
    f.X_canon, f.C, f.N = torch.ones(n, 3), torch.ones(n, 1), 1
    return f


def test_bad_arguments_raise_before_any_device_call():
    kfs, pin = [frame(0, 4, 5), frame(1, 4, 5)], (4.0, 4.0, 2.0, 1.5)
    for kw in (dict(neighbours=256), dict(neighbours=torch.zeros((2, 256), dtype=torch.int32)), dict(neighbours=-1),
               dict(depth_rtol=0.0), dict(depth_rtol=1.0), dict(depth_rtol=float("nan")), dict(min_views=-1),
               dict(max_conflicts=-1), dict(z_min=-1e-3), dict(z_min=float("nan"))):
        with pytest.raises(ValueError):
            consistency.multiview_support(kfs, pin, **kw)
    with pytest.raises(ValueError, match="4x5"):
        consistency.multiview_support([frame(0, 4, 5), frame(1, 5, 4)], pin)        # the same point count, another grid
    with pytest.raises(ValueError, match="pixels"):
        consistency.multiview_support([frame(0, 4, 5, n=21)], pin)                  # N != H * W
    with pytest.raises(ValueError):
        consistency.multiview_support(kfs, "guess")
    with pytest.raises(ValueError):
        consistency.multiview_support(kfs, (0.0, 4.0, 2.0, 1.5))
    with pytest.raises(RuntimeError, match="no CPU path"):
        consistency.multiview_support(kfs, pin)
    with pytest.raises(RuntimeError, match="no CPU path"):
        consistency.consistent_keyframes(kfs, pin, neighbours=None)


def test_no_keyframes_give_empty_tensors():
    empty = Frame(frame_id=0, img=torch.zeros(3, 4, 5), T_WC=torch.zeros(1, 8))     # no pointmap: skipped
    for kfs in ([], [empty]):
        s, c, conf = consistency.multiview_support(kfs, (4.0, 4.0, 2.0, 1.5))
        assert s.numel() == c.numel() == conf.numel() == 0
        assert s.dtype == torch.uint8 and c.dtype == torch.uint8 and conf.dtype == torch.float32
        assert consistency.consistent_keyframes(kfs, "estimate") == []


def test_re_exports_and_signatures():
    for n in ("multiview_support", "consistent_keyframes"):
        assert n in mast3r_utils.__all__ and n in consistency.__all__ and getattr(mast3r_utils, n) is getattr(consistency, n)
    from mast3r_slam.slam import SLAM
    E = inspect.Parameter.empty
    sig = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    assert sig(consistency.multiview_support)[:9] == [
        ("keyframes", E), ("K", E), ("neighbours", 8), ("c_conf_threshold", 1.5), ("depth_rtol", 0.03), ("min_views", 2),
        ("max_conflicts", 1), ("z_min", 1e-3), ("out", None)]
    for fn in (SLAM.reconstruction, SLAM.save_pointcloud, SLAM.mesh):
        assert sig(fn)[-1] == ("consistency", None)


def test_symbols_are_exported_and_the_abi_is_unchanged():
    names = [n for n in _ffi.declared_symbols() if n.startswith("m3_consistency")]
    assert sorted(names) == ["m3_consistency", "m3_consistency_launches", "m3_consistency_ws_bytes"]
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), n
    L = _ffi.lib()
    assert L.m3_abi_version() == 4000
    assert len(L.m3_consistency_launches.argtypes) == 0 and L.m3_consistency_launches() == 3
    assert L.m3_consistency_ws_bytes(1, 512 * 512) == 64 + 512 * 512 * 4
    assert L.m3_consistency_ws_bytes(256, 512 * 512) == 256 * 64 + 256 * 512 * 512 * 4
    assert L.m3_consistency_ws_bytes(0, 4) == 0 and L.m3_consistency_ws_bytes(-1, 4) == 0 and L.m3_consistency_ws_bytes(1, 0) == 0
    assert L.m3_consistency_ws_bytes(1 << 11, 1 << 20) == 0                     # K * N = 2^31
    one, big = 0x1000, 1 << 30                                                  # never dereferenced: every call below is refused
    call = lambda **k: L.m3_consistency(*[k.get(n, d) for n, d in (
        ("X", one), ("C", one), ("poses", one), ("Nk", one), ("K", 2), ("H", 4), ("W", 4), ("use", 1), ("thr", 1.5), ("fx", 4.0),
        ("fy", 4.0), ("cx", 1.5), ("cy", 1.5), ("nbr", one), ("V", 1), ("z_min", 1e-3), ("rtol", 0.03), ("min_views", 2),
        ("max_conflicts", 1), ("ws", one), ("ws_bytes", big), ("support", one), ("conflict", one), ("conf", one), ("stream", None))])
    for bad in (dict(X=None), dict(C=None), dict(poses=None), dict(Nk=None), dict(ws=None), dict(support=None), dict(conflict=None),
                dict(conf=None), dict(nbr=None), dict(V=256), dict(V=-1), dict(rtol=0.0), dict(rtol=1.0), dict(rtol=float("nan")),
                dict(z_min=-1.0), dict(z_min=float("nan")), dict(min_views=-1), dict(max_conflicts=-2), dict(use=2), dict(H=0),
                dict(H=1 << 16, W=1 << 16), dict(fx=0.0), dict(fy=float("inf")), dict(cx=float("nan")), dict(ws_bytes=64),
                dict(ws=one + 4), dict(conf=one + 4), dict(support=one + 1), dict(K=-1)):
        assert call(**bad) == -1, bad
    assert call(K=0, X=None, C=None, poses=None, Nk=None, nbr=None, ws=None, support=None, conflict=None, conf=None) == 0
