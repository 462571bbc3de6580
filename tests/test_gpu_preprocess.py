"""GPU: resize_img_device / m3_resize_crop_u8 against tests/resample_twin.py (pinned to PIL on the CPU by
tests/test_preprocess_host.py).  Every comparison is exact: every byte of the uint8 image, every bit of the float one."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_twin as twin  # noqa: E402

make_content = twin.make_content

from mast3r_slam import config, dataloader, model as M, preprocess, synthetic  # noqa: E402
from mast3r_slam.slam import SLAM  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _check_resize_img(a, size, square_ok, dev):
    raw, img = twin.resize_img(a, size, square_ok)
    out, tf = preprocess.resize_img_device(torch.from_numpy(a).to(dev), size, square_ok, return_transformation=True)
    u = out["unnormalized_img"]
    assert u.dtype == torch.uint8 and u.is_cuda and tuple(u.shape) == raw.shape and u.is_contiguous()
    nbad = int((u.cpu().numpy() != raw).sum())
    assert nbad == 0, f"{nbad} of {raw.size} bytes differ"
    assert out["img"].dtype == torch.float32 and tuple(out["img"].shape) == img.shape
    assert np.array_equal(_bits(out["img"]), img.view(np.uint32))
    assert out["true_shape"].dtype == torch.int32 and out["true_shape"].tolist() == [list(raw.shape[:2])]
    assert tf == preprocess.resize_geometry(a.shape[0], a.shape[1], size, square_ok)[3]
    return u


# (H, W), size, square_ok: LANCZOS down, BICUBIC up, both axes, pure crop, portrait, odd, 224, square both ways
CASES = [((480, 640), 512, False), ((720, 1280), 512, False), ((1080, 1920), 512, False), ((333, 517), 512, False),
         ((517, 333), 512, False), ((100, 37), 512, False), ((120, 160), 512, False), ((600, 600), 512, False),
         ((600, 600), 512, True), ((300, 300), 512, False), ((512, 384), 512, False), ((300, 512), 512, False),
         ((512, 300), 512, False), ((640, 480), 224, False), ((300, 700), 224, False), ((150, 100), 224, False),
         ((223, 223), 224, False), ((1080, 1920), 224, False)]


@pytest.mark.parametrize("content", ("noise", "extreme"))
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0][1]}x{c[0][0]}-{c[1]}-{int(c[2])}")
def test_resize_img_device_equals_twin(case, content, dev):
    (h, w), size, square_ok = case
    _check_resize_img(make_content(content, h, w, seed=h * 7 + w), size, square_ok, dev)


def test_smooth_content_and_constant_extremes(dev):
    _check_resize_img(make_content("smooth", 480, 640), 512, False, dev)
    _check_resize_img(make_content("smooth", 1080, 1920), 512, False, dev)
    for v in (0, 255):                                                       # the clamp must hold a flat image exactly
        u = _check_resize_img(np.full((240, 320, 3), v, np.uint8), 512, False, dev)
        assert int(u.min()) == v and int(u.max()) == v
    a = np.zeros((481, 643, 3), np.uint8)                                    # isolated 255 pixels / lines: negative lobes
    a[::5, ::7] = 255
    a[240] = 255
    _check_resize_img(a, 512, False, dev)
    _check_resize_img(255 - a, 512, False, dev)


# explicit targets through resize_crop: one axis only, both filters in both directions, crop boxes off the tile grid
DIRECT = [((480, 640), (640, 300), (0, 0, 640, 300)), ((480, 640), (500, 480), (0, 0, 500, 480)),
          ((480, 640), (512, 384), (16, 8, 496, 376)), ((333, 517), (512, 330), (3, 5, 510, 326)),
          ((100, 37), (189, 512), (1, 1, 188, 511)), ((200, 300), (300, 200), (7, 9, 206, 190)),
          ((720, 1280), (512, 288), (100, 50, 170, 51))]


@pytest.mark.parametrize("kind", ("lanczos", "bicubic"))
@pytest.mark.parametrize("case", DIRECT, ids=lambda c: f"{c[0][1]}x{c[0][0]}-{c[1][0]}x{c[1][1]}")
def test_resize_crop_one_axis_both_filters_any_box(case, kind, dev):
    (h, w), out_wh, box = case
    a = make_content("noise", h, w, seed=3)
    ref = twin.resize(a, out_wh, kind)[box[1]:box[3], box[0]:box[2]]
    u, f = preprocess.resize_crop(torch.from_numpy(a).to(dev)[None], out_wh, kind, box)
    assert tuple(u.shape) == (1,) + ref.shape and np.array_equal(u[0].cpu().numpy(), ref)
    assert np.array_equal(_bits(f[0]), ((ref.astype(np.float32) / 255.0 - 0.5) / 0.5).view(np.uint32))
    u2, f2 = preprocess.resize_crop(torch.from_numpy(a).to(dev)[None], out_wh, kind, box, want_float=False)
    assert f2 is None and torch.equal(u2, u)


def test_batch_positions_and_source_views(dev):
    frames = np.stack([make_content("noise", 480, 640, seed=s) for s in range(8)])
    alone = [preprocess.resize_img_device(torch.from_numpy(f).to(dev))["unnormalized_img"] for f in frames]
    out = preprocess.resize_img_device(torch.from_numpy(frames).to(dev))
    assert tuple(out["unnormalized_img"].shape) == (8, 384, 512, 3) and tuple(out["img"].shape) == (8, 384, 512, 3)
    for i in range(8):
        assert torch.equal(out["unnormalized_img"][i], alone[i]), i
    assert np.array_equal(alone[5].cpu().numpy(), twin.resize_img(frames[5], 512)[0])
    norm = ((out["unnormalized_img"].cpu().numpy().astype(np.float32) / 255.0 - 0.5) / 0.5)
    assert np.array_equal(_bits(out["img"]), norm.view(np.uint32))
    # a view at an odd byte offset, and a non-contiguous one (every second column of a wider image)
    flat = torch.zeros(480 * 640 * 3 + 7, dtype=torch.uint8, device=dev)
    flat[7:] = torch.from_numpy(frames[2]).to(dev).reshape(-1)
    odd = flat[7:].view(480, 640, 3)
    assert odd.data_ptr() % 16 != 0
    assert torch.equal(preprocess.resize_img_device(odd)["unnormalized_img"], alone[2])
    wide = torch.zeros((480, 1280, 3), dtype=torch.uint8, device=dev)
    wide[:, ::2] = torch.from_numpy(frames[3]).to(dev)
    strided = wide[:, ::2]
    assert not strided.is_contiguous()
    assert torch.equal(preprocess.resize_img_device(strided)["unnormalized_img"], alone[3])
    with pytest.raises(TypeError):
        preprocess.resize_img_device(torch.zeros((48, 64, 3), device=dev))            # float32: convert first


@pytest.mark.parametrize("hw", [(512, 8192), (8192, 768), (1200, 8192)], ids=lambda s: f"{s[1]}x{s[0]}")
def test_long_edge_8192(hw, dev):
    _check_resize_img(make_content("noise", hw[0], hw[1], seed=11), 512, False, dev)


def test_graph_capture_replays_on_new_data(dev):
    frames = [make_content("noise", 720, 1280, seed=20 + s) for s in range(3)]
    src = torch.from_numpy(frames[0]).to(dev)
    eager = [preprocess.resize_img_device(torch.from_numpy(f).to(dev)) for f in frames]      # also uploads the tables
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        preprocess.resize_img_device(src)                                                   # warm up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = preprocess.resize_img_device(src)
    for i in (1, 2):
        src.copy_(torch.from_numpy(frames[i]).to(dev))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out["unnormalized_img"], eager[i]["unnormalized_img"])
        assert np.array_equal(_bits(out["img"]), _bits(eager[i]["img"]))


@pytest.fixture(scope="module")
def net(dev):
    return M.Mast3rFull(weights=M.init_random_weights(M.TINY_CFG, seed=1), cfg=M.TINY_CFG, device=dev)


def test_encode_takes_the_device_output(net, dev):
    a = synthetic.textured_image(480, 640, 9)
    u = preprocess.resize_img_device(torch.from_numpy(a).to(dev))["unnormalized_img"]
    ref = torch.from_numpy(twin.resize_img(a, 512)[0]).to(dev)
    assert torch.equal(net.encode(u), net.encode(ref))
    batch = preprocess.resize_img_device(torch.from_numpy(np.stack([a, a[::-1].copy()])).to(dev))["unnormalized_img"]
    assert torch.equal(net.encode(batch[1]), net.encode(torch.from_numpy(twin.resize_img(a[::-1].copy(), 512)[0]).to(dev)))


def test_frames_generator_batches_and_flushes_on_a_shape_change(dev):
    raw = [make_content("noise", 240, 320, seed=s) for s in range(3)] + [make_content("noise", 300, 200, seed=9)]
    ds = dataloader.ArrayDataset(raw, timestamps=[0.5, 1.5, 2.5, 3.5])
    for batch in (1, 2, 8):
        got = list(ds.frames(dev, batch=batch))
        assert [t for t, _ in got] == [0.5, 1.5, 2.5, 3.5]
        for (_, g), a in zip(got, raw):
            assert g.is_cuda and g.dtype == torch.uint8 and np.array_equal(g.cpu().numpy(), twin.resize_img(a, 512)[0])
    assert tuple(next(iter(ds.frames(dev, size=224)))[1].shape) == (224, 224, 3)


def test_run_dataset_equals_run_on_twin_frames(net, dev):
    """640x480 frames through SLAM.run_dataset (resized on the device) against SLAM.run on the same frames resized by
    the twin on the host: the network sees identical bytes, so every result is identical."""
    raw = [synthetic.textured_image(480, 640, 40 + k) for k in range(4)]
    ts = [0.1 * k for k in range(4)]
    config.set_config({})
    try:
        a = SLAM(net)
        out_a = a.run_dataset(dataloader.ArrayDataset(raw, timestamps=ts))
        b = SLAM(net)
        out_b = b.run([(t, torch.from_numpy(twin.resize_img(f, 512)[0])) for t, f in zip(ts, raw)])
    finally:
        config.reset_config()
    assert len(a.keyframes) == len(b.keyframes) >= 1
    assert out_a["timestamps"] == out_b["timestamps"] == ts
    assert out_a["keyframe_indices"] == out_b["keyframe_indices"]
    assert out_a["poses"].shape == (4, 8) and torch.equal(out_a["poses"], out_b["poses"])
    assert out_a["points"].shape == (len(a.keyframes) * 384 * 512, 3) and torch.equal(out_a["points"], out_b["points"])
    for ka, kb in zip(a.keyframes._frames, b.keyframes._frames):
        assert torch.equal(ka.img, kb.img.to(dev)) and torch.equal(ka.T_WC, kb.T_WC)


def test_run_dataset_adjusts_the_intrinsics(net, dev):
    K = torch.tensor([[525.0, 0, 319.5], [0, 525.0, 239.5], [0, 0, 1]])
    s = SLAM(net, K=K)
    s.run_dataset(dataloader.ArrayDataset([synthetic.textured_image(480, 640, 1)]))
    want = preprocess.adjust_intrinsics(K, preprocess.resize_geometry(480, 640, 512)[3])
    assert torch.equal(s.keyframes.get_intrinsics(), want) and float(want[0, 0]) == 525.0 / 1.25
    assert torch.equal(s.keyframes[0].K, want)
