"""GPU: the focal estimate (csrc/intrinsics.hip through the C ABI and intrinsics.estimate_focal) against its float64
twin (tests/focal_twin.py).

The count must be equal; the two focals and the mean residual must agree within a relative 1e-9: twin and kernel differ
only in the order of float64 sums of at most 2^18 terms (2^18 * 2^-53 = 3e-11 per sum), the Weiszfeld map is a
contraction near its fixed point, so the difference does not grow over the passes; 1e-9 leaves a factor 30.  Load
paths, the validity rule, degenerate rows, determinism and graph capture are exact."""
import functools

import numpy as np
import pytest
import torch

import focal_twin as FT
import render_scenes as RS
from mast3r_slam import _ffi, intrinsics, render

pytestmark = pytest.mark.gpu
RTOL = 1e-9
TILE = 4096                                                                   # pixels per workgroup (csrc/intrinsics.hip)


@functools.lru_cache(maxsize=None)
def scene(H, W, focals, seed, nks=None, **kw):
    return FT.pinhole_scene(H, W, list(focals), seed, nks=nks, **kw)


@functools.lru_cache(maxsize=None)
def twin(H, W, focals, seed, nks=None, thr=1.5, z_min=0.0, iters=10):
    return FT.focal_twin_map(scene(H, W, focals, seed, nks), (H, W), thr=thr, z_min=z_min, iters=iters)


def via_abi(sc, size, dev, thr=1.5, z_min=0.0, iters=10, pp=None, offset_x=False):
    """[K,4] through m3_focal_estimate on tables built here; offset_x: every X starts 4 bytes past a 16-byte boundary."""
    K, N = sc["K"], sc["N"]
    H, W = size
    Xs = []
    for k in range(K):
        buf = torch.empty(3 * N + 4, dtype=torch.float32, device=dev)
        x = buf[1:3 * N + 1] if offset_x else buf[:3 * N]
        x.copy_(torch.from_numpy(sc["X"][k].reshape(-1)))
        assert x.data_ptr() % 16 == (4 if offset_x else 0)
        Xs.append(x)
    Cs = [torch.from_numpy(sc["C"][k]).to(dev) for k in range(K)]
    table = torch.tensor([[t.data_ptr() for t in Xs], [t.data_ptr() for t in Cs]], dtype=torch.int64).to(dev)
    nk = torch.from_numpy(np.asarray(sc["Nk"], dtype=np.int32)).to(dev)
    L = _ffi.lib()
    ws_bytes = int(L.m3_focal_ws_bytes(K, N))
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.full((K, 4), -7.0, dtype=torch.float64, device=dev)
    cx, cy = ((W - 1) / 2.0, (H - 1) / 2.0) if pp is None else pp
    use, t = (0, 0.0) if thr is None else (1, float(thr))
    _ffi.call("m3_focal_estimate", _ffi.ptr(table[0]), _ffi.ptr(table[1]), _ffi.ptr(nk), K, N, H, W, use, t, cx, cy,
              float(z_min), iters, _ffi.ptr(ws), ws_bytes, _ffi.ptr(out), _ffi.stream_ptr())
    return out.cpu().numpy()


def via_module(sc, dev, **kw):
    out = intrinsics.estimate_focal(RS.frames_of(sc, dev), **kw)
    assert out.dtype == torch.float64 and out.shape == (sc["K"], 4) and out.is_cuda
    return out.cpu().numpy()


def check(got, want, label):
    """Count equal; the other three columns NaN where the twin's are, else within RTOL."""
    assert got.shape == want.shape
    print(f"{label}: counts {got[:, 2].astype(np.int64).tolist()}")
    assert np.array_equal(got[:, 2], want[:, 2])
    for col, name in ((0, "focal"), (1, "lsq focal"), (3, "residual")):
        g, w = got[:, col], want[:, col]
        assert np.array_equal(np.isnan(g), np.isnan(w)), (name, g, w)
        ok = ~np.isnan(w)
        rel = np.abs(g[ok] - w[ok]) / np.abs(w[ok])
        print(f"{label}: {name} {g.tolist()} max relative difference to the twin {rel.max() if rel.size else 0.0:.3g}")
        assert (rel <= RTOL).all(), (name, g, w)


# ---- 1. parity with the twin -----------------------------------------------------------------------------------------
PARITY = [
    (37, 53, (30.0,), None),                    # N = 1961, odd: scalar loads and a ragged only tile
    (64, 64, (55.0,), None),                    # one exact tile
    (17, 241, (150.0,), None),                  # N = TILE + 1: a second tile of one pixel, scalar loads
    (128, 160, (120.0,), None),                 # five tiles
    (37, 53, (30.0, 45.0, 38.0), (1, 2, 5)),    # three different keyframes, fusion counts 1, 2, 5
    (512, 512, (400.0, 520.0), (1, 3)),         # the production size: 64 tiles per keyframe
]


@pytest.mark.parametrize("H,W,focals,nks", PARITY)
def test_parity_with_the_twin(dev, H, W, focals, nks):
    assert (H, W) != (64, 64) or H * W == TILE
    assert (H, W) != (17, 241) or H * W == TILE + 1
    sc, want = scene(H, W, focals, 3, nks), twin(H, W, focals, 3, nks)
    assert (np.abs(want[:, 0] - np.asarray(focals)) / np.asarray(focals) < 0.005).all()     # the scene is meaningful
    abi = via_abi(sc, (H, W), dev)
    check(abi, want, f"{H}x{W} K={len(focals)} abi")
    mod = via_module(sc, dev)
    assert mod.tobytes() == abi.tobytes()                                    # the module adds nothing to the numbers
    sized = via_module(sc, dev, size=(H, W), principal_point=((W - 1) / 2.0, (H - 1) / 2.0))
    assert sized.tobytes() == abi.tobytes()                                  # the defaults are what they say


def test_principal_point_z_min_and_iteration_count_reach_the_kernel(dev):
    H, W, focals = 48, 64, (70.0, 60.0)
    sc = scene(H, W, focals, 5)
    for kw in (dict(pp=(30.25, 25.5)), dict(z_min=2.0), dict(iters=1), dict(iters=64), dict(thr=2.25)):
        want = FT.focal_twin_map(sc, (H, W), **kw)
        check(via_abi(sc, (H, W), dev, **kw), want, f"48x64 {kw}")
    assert FT.focal_twin_map(sc, (H, W), z_min=2.0)[0, 2] < twin(H, W, focals, 5)[0, 2]
    mod = intrinsics.estimate_focal(RS.frames_of(sc, dev), principal_point=(30.25, 25.5), z_min=2.0, iters=3,
                                    c_conf_threshold=2.25).cpu().numpy()
    check(mod, FT.focal_twin_map(sc, (H, W), pp=(30.25, 25.5), z_min=2.0, iters=3, thr=2.25), "48x64 module keywords")


def test_scalar_and_vector_loads_give_the_same_bits(dev):
    sc = scene(64, 64, (55.0, 80.0), 7)
    a = via_abi(sc, (64, 64), dev)
    b = via_abi(sc, (64, 64), dev, offset_x=True)
    assert a.tobytes() == b.tobytes()
    check(b, twin(64, 64, (55.0, 80.0), 7), "64x64 K=2, X offset by 4 bytes")


# ---- 2. the validity rule --------------------------------------------------------------------------------------------
def test_exactly_the_valid_pixels_contribute(dev):
    H, W, Z_MIN = 37, 53, 0.25
    base = scene(H, W, (30.0,), 11, (2,))
    sc = dict(base, X=base["X"].copy(), C=base["C"].copy())
    X, C = sc["X"][0], sc["C"][0]
    px = np.arange(16) * 117 + 40                                             # 16 pixels spread over the image
    C[px] = np.float32(2.5) * 2                                               # each would count if its defect went unseen
    X[px, 2] = np.abs(X[px, 2]) + 1                                           # (and is in front of z_min to begin with)
    for i, (comp, val) in enumerate((c, v) for c in range(3) for v in (np.nan, np.inf, -np.inf)):
        X[px[i], comp] = val
    X[px[9], 2], X[px[10], 2], X[px[11], 2] = 0.0, -1.5, Z_MIN                # z = 0, z < 0, z = z_min exactly
    C[px[12]] = np.float32(1.5) * 2                                           # C / N exactly at the threshold
    C[px[13]] = np.nan
    X[px[14], 2] = np.nextafter(np.float32(Z_MIN), np.float32(1))             # the first z that passes
    C[px[15]] = np.nextafter(np.float32(3.0), np.float32(4))                  # the first C that passes (3 / 2 = 1.5)
    clean = dict(sc, X=sc["X"].copy(), C=sc["C"].copy())
    clean["X"][0][px[:14]] = base["X"][0][px[:14]]
    clean["X"][0][px[:14], 2] = 2.0
    clean["C"][0][px[:14]] = 5.0
    for thr in (1.5, None):
        want = FT.focal_twin_map(sc, (H, W), thr=thr, z_min=Z_MIN)
        all_in = FT.focal_twin_map(clean, (H, W), thr=thr, z_min=Z_MIN)
        assert all_in[0, 2] - want[0, 2] == (14 if thr is not None else 12)   # without the test the two C defects count
        check(via_abi(sc, (H, W), dev, thr=thr, z_min=Z_MIN), want, f"planted defects thr={thr}")
    mod = intrinsics.estimate_focal(RS.frames_of(sc, dev), c_conf_threshold=None, z_min=Z_MIN).cpu().numpy()
    check(mod, FT.focal_twin_map(sc, (H, W), thr=None, z_min=Z_MIN), "planted defects, module, no confidence test")


# ---- 3. degenerate rows ----------------------------------------------------------------------------------------------
def test_keyframes_without_information(dev):
    H, W = 5, 7
    base = scene(H, W, (6.0, 6.0, 6.0), 13)
    sc = dict(base, X=base["X"].copy(), C=base["C"].copy())
    sc["C"][0][:] = 0.0                                                       # keyframe 0: no valid pixel
    sc["C"][1][:] = 0.0                                                       # keyframe 1: only the principal point, on the axis
    centre = 2 * W + 3
    sc["C"][1][centre], sc["X"][1][centre] = 2.0, (0.0, 0.0, 2.0)
    sc["C"][2][:] = 2.0
    got = via_abi(sc, (H, W), dev)
    print(got.tolist())
    assert np.isnan(got[0, [0, 1, 3]]).all() and got[0, 2] == 0
    assert np.isnan(got[1, [0, 1]]).all() and got[1, 2] == 1                  # 0 / 0
    assert np.isfinite(got[2]).all() and got[2, 2] == H * W
    check(got, FT.focal_twin_map(sc, (H, W)), "5x7 degenerate")


def test_noise_free_scenes_meet_the_residual_floor(dev):
    H, W, f = 48, 64, 70.0
    sc = scene(H, W, (f,), 17, None, out_frac=0.0, noise=0.0)
    got = via_abi(sc, (H, W), dev, thr=None)
    print(f"noise-free recipe: {got.tolist()}, twin {FT.focal_twin_map(sc, (H, W), thr=None).tolist()}")
    assert np.isfinite(got).all() and abs(got[0, 0] - f) <= 1e-6 and abs(got[0, 1] - f) <= 1e-6 and got[0, 2] == H * W
    assert 0.0 <= got[0, 3] < 1e-4
    # every operation exact (f = 64, z = 2, integer u and v): every residual is exactly 0 and takes the 1e-8 floor
    H, W, f = 33, 65, 64.0
    v, u = np.meshgrid(np.arange(H) - (H - 1) / 2.0, np.arange(W) - (W - 1) / 2.0, indexing="ij")
    X = np.stack([u / f * 2.0, v / f * 2.0, np.full_like(u, 2.0)], axis=2).reshape(1, -1, 3).astype(np.float32)
    ex = dict(sc, X=X, C=np.full((1, H * W), 2.0, dtype=np.float32), N=H * W, H=H, W=W, img=np.zeros((1, H * W, 3), dtype=np.uint8))
    got = via_abi(ex, (H, W), dev)
    assert got.tolist() == [[64.0, 64.0, float(H * W), 0.0]]


def test_zero_iterations_return_the_least_squares_focal(dev):
    sc = scene(37, 53, (30.0, 45.0, 38.0), 3, (1, 2, 5))
    got = via_abi(sc, (37, 53), dev, iters=0)
    assert got[:, 0].tobytes() == got[:, 1].tobytes()
    check(got, twin(37, 53, (30.0, 45.0, 38.0), 3, (1, 2, 5), iters=0), "37x53 iters=0")
    assert via_abi(sc, (37, 53), dev, iters=10)[:, 1].tobytes() == got[:, 1].tobytes()      # pass 0 is the same pass


# ---- 4. determinism, independence of the batch, graph capture, empty map ------------------------------------------
def test_two_calls_and_any_batch_give_identical_bytes(dev):
    H, W, focals, nks = 128, 160, (120.0, 90.0, 150.0), (1, 2, 5)
    sc = scene(H, W, focals, 19, nks)
    frames = RS.frames_of(sc, dev)
    a, b = intrinsics.estimate_focal(frames), intrinsics.estimate_focal(frames)
    assert torch.equal(a, b) and a.data_ptr() != b.data_ptr()
    check(a.cpu().numpy(), twin(H, W, focals, 19, nks), "128x160 K=3")
    for k in range(3):
        alone = intrinsics.estimate_focal(frames[k:k + 1])
        assert alone.shape == (1, 4) and alone.cpu().numpy().tobytes() == a[k:k + 1].cpu().numpy().tobytes()
    pair = intrinsics.estimate_focal([frames[2], frames[0]])
    assert torch.equal(pair, a[[2, 0]])


def test_graph_replay_equals_the_eager_call(dev):
    H, W, focals, nks = 128, 160, (120.0, 90.0, 150.0), (1, 2, 5)
    frames = RS.frames_of(scene(H, W, focals, 19, nks), dev)
    want = intrinsics.estimate_focal(frames)
    tables = render.map_tables(frames)                                        # host-to-device copies stay outside the capture
    out = torch.empty((3, 4), dtype=torch.float64, device=dev)
    ws = torch.empty(intrinsics.workspace_bytes(3, H * W), dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                             # warm-up outside the capture
        intrinsics.estimate_focal(tables, out=out, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(out, want)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                             # one stream: a serial chain of launches
        got = intrinsics.estimate_focal(tables, out=out, workspace=ws)
    assert got is out
    for _ in range(2):
        out.fill_(-1.0)
        ws.fill_(255)
        graph.replay()
        assert torch.equal(out, want)


def test_an_empty_map_makes_no_launch(dev, monkeypatch):
    L = _ffi.lib()
    assert L.m3_focal_launches(0) == 3 and L.m3_focal_launches(10) == 13 and L.m3_focal_launches(64) == 67
    out = torch.full((2, 4), -7.0, dtype=torch.float64, device=dev)
    ws = torch.empty(64, dtype=torch.uint8, device=dev)
    nk = torch.ones(2, dtype=torch.int32, device=dev)
    X, C = torch.ones((2, 20, 3), dtype=torch.float32, device=dev), torch.full((2, 20), 2.0, dtype=torch.float32, device=dev)
    tab = torch.tensor([[X[0].data_ptr(), X[1].data_ptr()], [C[0].data_ptr(), C[1].data_ptr()]], dtype=torch.int64).to(dev)
    _ffi.call("m3_focal_estimate", _ffi.ptr(tab[0]), _ffi.ptr(tab[1]), _ffi.ptr(nk), 0, 20, 4, 5, 1, 1.5, 2.0, 1.5, 0.0, 10,
              _ffi.ptr(ws), 64, _ffi.ptr(out), _ffi.stream_ptr())
    torch.cuda.synchronize()
    assert (out == -7.0).all()

    def no_call(*a, **k):
        raise AssertionError("an empty map must not reach the library")

    monkeypatch.setattr(_ffi, "call", no_call)
    got = intrinsics.estimate_focal([])
    assert got.shape == (0, 4) and got.dtype == torch.float64 and got.is_cuda
    assert intrinsics.estimate_focal([], size=(4, 5), iters=0).shape == (0, 4)
