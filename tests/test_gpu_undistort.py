"""GPU: camera.undistort_device / m3_remap_bilinear_u8 against tests/undistort_twin.py (pinned to the meaning of the camera
model by tests/test_camera_host.py), and the calibrated path of Dataset.frames / SLAM.run_dataset.  Every comparison
is exact and covers every byte."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_twin  # noqa: E402
import undistort_twin as twin  # noqa: E402

from mast3r_slam import _ffi, camera, config, dataloader, model as M, synthetic  # noqa: E402
from mast3r_slam.camera import CameraModel  # noqa: E402
from mast3r_slam.slam import SLAM  # noqa: E402

pytestmark = pytest.mark.gpu

EUROC = dict(width=752, height=480, K=[458.654, 457.296, 367.215, 248.375],
             distortion=(-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05), model="radtan")
TUM1 = dict(width=640, height=480, K=[517.3, 516.5, 318.6, 255.3], distortion=(0.2624, -0.9531, -0.0054, 0.0026, 1.1633),
            model="radtan")
SMALL = dict(width=61, height=45, K=[48, 47, 30.2, 21.7], distortion=(-0.25, 0.06, 0.001, -0.002), model="radtan")
HD = dict(EUROC, width=1920, height=1080, K=[458.654 * 1920 / 752, 457.296 * 1080 / 480, 367.215 * 1920 / 752, 248.375 * 1080 / 480])
SENT = twin.SENTINEL


def _twin_table(spec, K_new, out_wh):
    return twin.table(spec["model"], spec["K"], spec["distortion"], K_new, out_wh)


def _same(got, want):
    assert got.dtype == torch.uint8 and got.is_cuda and got.is_contiguous() and tuple(got.shape) == want.shape
    nbad = int((got.cpu().numpy() != want).sum())
    assert nbad == 0, f"{nbad} of {want.size} bytes differ"


# spec, K_new, out_size (W, H) or None
CASES = {
    "small-same": (SMALL, "same", None),                       # a barrel lens: "same" keeps every tap inside
    "small-wide": (SMALL, [36.0, 35.0, 29.0, 23.0], None),     # a shorter focal length: taps outside on all four sides
    "small-inner": (SMALL, "inner", None),
    "small-37x29": (SMALL, [30.0, 31.0, 17.5, 14.2], (37, 29)),  # Wo % 4 != 0, Ws * 3 and Wo * 3 no multiples of 16
    "tum1-inner": (TUM1, "inner", None),
    "euroc-inner": (EUROC, "inner", None),
    "euroc-1920x1080": (HD, "inner", None),
}


@pytest.mark.parametrize("content", ("noise", "extreme"))
@pytest.mark.parametrize("case", list(CASES))
def test_undistort_device_equals_twin(case, content, dev):
    spec, K_new, out_size = CASES[case]
    cam = CameraModel(**spec)
    src = twin.make_content(content, spec["height"], spec["width"], seed=len(case))
    out_wh = out_size or (spec["width"], spec["height"])
    tab = _twin_table(spec, cam.new_camera_matrix(K_new, out_wh), out_wh)
    got = camera.undistort_device(torch.from_numpy(src).to(dev), cam, K_new, out_size)
    _same(got, twin.remap(src, tab))
    if case in ("small-same", "small-wide"):                             # the border byte reaches the outside taps
        ix, iy = tab[..., 0] >> 8, tab[..., 1] >> 8
        if case == "small-wide":                                         # wholly outside on each side, and half outside
            assert (ix < -1).any() and (ix > 61).any() and (iy < -1).any() and (iy > 45).any()
            assert ((ix == -1) | (ix == 60) | (iy == -1) | (iy == 44)).any() and twin.taps_inside(tab, 45, 61).any()
        _same(camera.undistort_device(torch.from_numpy(src).to(dev), cam, K_new, border=200), twin.remap(src, tab, 200))


def _remap(src, tab, dev, border=0):
    got = camera.remap_bilinear(torch.from_numpy(src).to(dev)[None], torch.from_numpy(np.ascontiguousarray(tab, np.int32)).to(dev), border)
    _same(got[0], twin.remap(src, np.asarray(tab, np.int32), border))
    return got[0].cpu().numpy()


@pytest.mark.parametrize("hw", [(45, 61), (32, 64), (5, 3), (130, 517)], ids=lambda s: f"{s[1]}x{s[0]}")
def test_hand_made_tables(hw, dev):
    h, w = hw
    v, u = np.mgrid[0:h, 0:w]
    ident = np.stack([u << 8, v << 8], -1)
    checker = (((u + v) % 2) * 255).astype(np.uint8)[..., None].repeat(3, -1)
    for src in (twin.make_content("noise", h, w, seed=1), twin.make_content("extreme", h, w), checker):
        assert np.array_equal(_remap(src, ident, dev), src)                                  # identity
        half = _remap(src, ident + 128, dev)                                                 # the rounded four-pixel mean
        s = src.astype(np.int64)
        if h > 1 and w > 1:
            mean4 = (s[:-1, :-1] + s[:-1, 1:] + s[1:, :-1] + s[1:, 1:] + 2) >> 2
            assert np.array_equal(half[:-1, :-1], mean4)
        for border in (0, 200):
            assert (_remap(src, np.full((h, w, 2), SENT), dev, border) == border).all()      # sentinels only
            far = ident.copy()
            far[0::4, :, 0] = -(1 << 27)                                                     # far outside on the four sides
            far[1::4, :, 0] = (1 << 27)
            far[2::4, :, 1] = -(1 << 27)
            far[3::4, :, 1] = (1 << 28) - 1
            far[:, 0] = (SENT, 5 << 8)                                                       # half a sentinel is outside too
            assert (_remap(src, far, dev, border) == border).all()
            # the last pixel with zero weights on its outside taps, and coordinates just below zero (ix = -1, a = 255)
            edge = ident.copy()
            edge[:, ::2] = ((w - 1) << 8, (h - 1) << 8)
            out = _remap(src, edge, dev, border)
            assert (out[:, ::2] == src[h - 1, w - 1]).all()
            neg = ident.copy()
            neg[..., 0] -= 1
            neg[::2, :, 1] -= 1
            out = _remap(src, neg, dev, border)
            # row 1, column 0: only x is below zero, so p00 (weight 256) is outside and p01 = src[1][0] has weight 255 * 256
            assert np.array_equal(out[1, 0], (border * 256 + s[1, 0] * 255 * 256 + (1 << 15)) >> 16)


def test_batch_positions_views_and_repeatability(dev):
    cam = CameraModel(**TUM1)
    frames = np.stack([twin.make_content("noise", 480, 640, seed=s) for s in range(3)])
    alone = [camera.undistort_device(torch.from_numpy(f).to(dev), cam) for f in frames]
    both = camera.undistort_device(torch.from_numpy(frames).to(dev), cam)
    assert tuple(both.shape) == (3, 480, 640, 3)
    for i in range(3):
        assert torch.equal(both[i], alone[i]), i
    _same(alone[2], twin.remap(frames[2], _twin_table(TUM1, cam.new_camera_matrix("inner"), (640, 480))))
    assert torch.equal(camera.undistort_device(torch.from_numpy(frames).to(dev), cam), both)       # two calls, same bytes
    flat = torch.zeros(480 * 640 * 3 + 7, dtype=torch.uint8, device=dev)
    flat[7:] = torch.from_numpy(frames[1]).to(dev).reshape(-1)
    odd = flat[7:].view(480, 640, 3)
    assert odd.data_ptr() % 16 != 0
    assert torch.equal(camera.undistort_device(odd, cam), alone[1])
    wide = torch.zeros((480, 1280, 3), dtype=torch.uint8, device=dev)
    wide[:, ::2] = torch.from_numpy(frames[0]).to(dev)
    assert torch.equal(camera.undistort_device(wide[:, ::2], cam), alone[0])                       # not contiguous
    with pytest.raises(TypeError):
        camera.undistort_device(torch.zeros((480, 640, 3), device=dev), cam)                       # float32
    with pytest.raises(ValueError, match="640x480"):
        camera.undistort_device(torch.zeros((48, 64, 3), dtype=torch.uint8, device=dev), cam)      # not this camera's size
    # no distortion and the camera's own matrix: the input comes back, nothing is launched
    flat_cam = CameraModel(640, 480, TUM1["K"], (0, 0, 0, 0, 0), "radtan")
    src = torch.from_numpy(frames[0]).to(dev)
    assert camera.undistort_device(src, flat_cam) is src and camera.undistort_device(src, flat_cam, "same") is src
    _same(camera.undistort_device(src, flat_cam, [400.0, 400.0, 300.0, 200.0]),
          twin.remap(frames[0], _twin_table(dict(TUM1, distortion=()), [400.0, 400.0, 300.0, 200.0], (640, 480))))


def test_graph_capture_replays_on_new_data(dev):
    cam = CameraModel(**EUROC)
    frames = [twin.make_content("noise", 480, 752, seed=30 + s) for s in range(3)]
    tab = _twin_table(EUROC, cam.new_camera_matrix("inner"), (752, 480))
    src = torch.from_numpy(frames[0]).to(dev)
    camera.undistort_device(src, cam)                                                    # uploads the table
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        camera.undistort_device(src, cam)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = camera.undistort_device(src, cam)
    for i in (1, 2):
        src.copy_(torch.from_numpy(frames[i]).to(dev))
        g.replay()
        torch.cuda.synchronize()
        _same(out, twin.remap(frames[i], tab))


def test_frames_of_a_calibrated_dataset_equal_the_two_twins(dev):
    cam = CameraModel(**TUM1)
    raw = [twin.make_content("noise", 480, 640, seed=50 + s) for s in range(4)]
    tab = _twin_table(TUM1, cam.new_camera_matrix("inner"), (640, 480))
    want = [resample_twin.resize_img(twin.remap(a, tab), 512)[0] for a in raw]            # computed once, shared below
    ds = dataloader.ArrayDataset(raw, timestamps=[0.5, 1.5, 2.5, 3.5], calibration=cam)
    for batch in (1, 3):
        got = list(ds.frames(dev, batch=batch))
        assert [t for t, _ in got] == [0.5, 1.5, 2.5, 3.5]
        for (_, g), w in zip(got, want):
            _same(g, w)
    # undistort=False, or the optional config key, leaves the frames as an uncalibrated dataset yields them
    plain = [g for _, g in dataloader.ArrayDataset(raw[:1]).frames(dev)]
    assert torch.equal(next(iter(ds.frames(dev, undistort=False)))[1], plain[0])
    config.set_config({"dataset": {"undistort": False}})
    try:
        assert torch.equal(next(iter(ds.frames(dev)))[1], plain[0])
    finally:
        config.reset_config()
    config.set_config({"dataset": {"new_camera_matrix": "same"}})
    try:
        _same(next(iter(ds.frames(dev)))[1], resample_twin.resize_img(twin.remap(raw[0], _twin_table(TUM1, TUM1["K"], (640, 480))), 512)[0])
    finally:
        config.reset_config()
    # a shape change between frames: the batch before it is flushed, the frame that is not the calibration's size raises
    mixed = dataloader.ArrayDataset(raw[:2] + [twin.make_content("noise", 300, 200, seed=9)], calibration=cam)
    for batch in (1, 3):
        it = mixed.frames(dev, batch=batch)
        _same(next(it)[1], want[0])
        _same(next(it)[1], want[1])
        with pytest.raises(ValueError, match="640x480.*200x300"):
            next(it)


def test_a_calibration_without_distortion_changes_nothing(dev):
    raw = [twin.make_content("noise", 240, 320, seed=s) for s in range(3)]
    flat = CameraModel(320, 240, [260.0, 261.0, 159.5, 119.5], (0, 0, 0, 0), "radtan")
    a = list(dataloader.ArrayDataset(raw).frames(dev, batch=2))
    b = list(dataloader.ArrayDataset(raw, calibration=flat).frames(dev, batch=2))
    c = list(dataloader.ArrayDataset(raw, calibration=CameraModel(320, 240, [260.0, 261.0, 159.5, 119.5])).frames(dev, batch=2))
    for (_, x), (_, y), (_, z), r in zip(a, b, c, raw):
        assert torch.equal(x, y) and torch.equal(x, z)
        _same(x, resample_twin.resize_img(r, 512)[0])


@pytest.fixture(scope="module")
def net(dev):
    return M.Mast3rFull(weights=M.init_random_weights(M.TINY_CFG, seed=1), cfg=M.TINY_CFG, device=dev)


def test_run_dataset_takes_the_intrinsics_of_a_calibrated_dataset(net, dev):
    cam = CameraModel(**TUM1)
    raw = [synthetic.textured_image(480, 640, 40 + k) for k in range(4)]
    ds = dataloader.ArrayDataset(raw, timestamps=[0.1 * k for k in range(4)], calibration=cam)
    config.set_config({"use_calib": True})
    try:
        s = SLAM(net)
        out = s.run_dataset(ds)
        want = ds.intrinsics(512)
    finally:
        config.reset_config()
    assert out["poses"].shape == (4, 8) and len(out["timestamps"]) == 4 and len(s.keyframes) >= 1
    assert torch.isfinite(out["poses"]).all()
    for K in (s.keyframes.get_intrinsics(), s.factor_graph.K, s.keyframes[0].K):
        assert np.array_equal(np.asarray(K.cpu()), want)
    # without use_calib the keyframes still carry the dataset's intrinsics; the factor graph stays uncalibrated
    s2 = SLAM(net)
    s2.run_dataset(dataloader.ArrayDataset(raw[:1], calibration=cam))
    assert np.array_equal(np.asarray(s2.keyframes.get_intrinsics()), want) and s2.factor_graph.K is None
    with pytest.raises(ValueError, match=r"(?s)K.*calibration"):
        SLAM(net, K=torch.eye(3)).run_dataset(ds)


def test_c_abi_refuses_bad_arguments(dev):
    L = _ffi.lib()
    src = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=dev)
    tab = torch.zeros((8, 8, 2), dtype=torch.int32, device=dev)
    dst = torch.full((1, 8, 8, 3), 7, dtype=torch.uint8, device=dev)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    f = L.m3_remap_bilinear_u8
    st = ctypes.c_void_p(_ffi.stream_ptr())
    assert f(None, p(tab), p(dst), 1, 8, 8, 8, 8, 0, st) == -1 and f(p(src), None, p(dst), 1, 8, 8, 8, 8, 0, st) == -1
    assert f(p(src), p(tab), None, 1, 8, 8, 8, 8, 0, st) == -1
    assert f(p(src, 3), p(tab), p(dst), 1, 8, 8, 8, 8, 0, st) == -1 and f(p(src), p(tab, 8), p(dst), 1, 8, 8, 8, 8, 0, st) == -1
    for bad in ((0, 8, 8, 8, 8, 0), (1, 0, 8, 8, 8, 0), (1, 8, 8, -8, 8, 0), (1, 8, 8, 8, 0, 0), (1, 8, 8, 8, 8, 256), (65536, 8, 8, 8, 8, 0)):
        assert f(p(src), p(tab), p(dst), *bad, st) == -1, bad
    torch.cuda.synchronize()
    assert (dst == 7).all()                                                              # nothing was launched
    assert f(p(src), p(tab), p(dst), 1, 8, 8, 8, 8, 0, st) == 0
    torch.cuda.synchronize()
    assert (dst == 0).all()
