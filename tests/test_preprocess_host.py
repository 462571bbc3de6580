"""CPU: the host side of the device preprocessing and the dataset readers.  tests/resample_twin.py (the numpy yardstick
of the GPU tests) is pinned to PIL.Image.resize byte for byte; the product's coefficient tables equal the twin's; the
geometry function equals resize_img's; the readers follow the reference's detection, ordering and timestamps."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_twin as twin  # noqa: E402

from mast3r_slam import _ffi, config, dataloader, mast3r_utils, preprocess  # noqa: E402

# (source H, W) -> target (W, H): down- and up-scaling, odd sizes, portrait
SHAPES = [((480, 640), (512, 384)), ((720, 1280), (512, 288)), ((1080, 1920), (512, 288)), ((333, 517), (512, 330)),
          ((100, 37), (189, 512)), ((120, 160), (512, 384)), ((600, 600), (512, 512)), ((640, 480), (384, 512)),
          ((517, 333), (330, 512))]
ONE_AXIS = [((480, 640), (640, 300)), ((480, 640), (500, 480)), ((200, 300), (300, 333)), ((200, 300), (411, 200))]
CONTENT = ("noise", "smooth", "extreme")


make_content = twin.make_content


@pytest.mark.parametrize("content", CONTENT)
@pytest.mark.parametrize("shape", SHAPES + ONE_AXIS, ids=lambda s: f"{s[0][1]}x{s[0][0]}-{s[1][0]}x{s[1][1]}")
def test_twin_equals_pil_byte_for_byte(shape, content):
    from PIL import Image
    (h, w), out = shape
    a = make_content(content, h, w)
    for kind, pil_kind in (("lanczos", Image.LANCZOS), ("bicubic", Image.BICUBIC)):
        ref = np.asarray(Image.fromarray(a).resize(out, pil_kind))
        got = twin.resize(a, out, kind)
        assert got.shape == ref.shape and int((got != ref).sum()) == 0, (shape, content, kind)


def test_resample_tables_equal_the_twin_and_are_cached():
    sizes = [(640, 512), (1920, 512), (1080, 288), (517, 512), (333, 330), (37, 189), (100, 512), (8192, 512), (4608, 288),
             (600, 512), (480, 384), (160, 512), (512, 511), (511, 512), (7, 3), (3, 7), (1, 5), (5, 1)]
    for i, o in sizes:
        for kind in ("lanczos", "bicubic"):
            b, k = preprocess.resample_tables(i, o, kind)
            bt, kt = twin.coeffs(i, o, kind)
            assert b.dtype == np.int32 and k.dtype == np.int32 and b.shape == (o, 2)
            assert np.array_equal(b, bt) and np.array_equal(k, kt), (i, o, kind)
            assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= i).all() and (b[:, 1] <= k.shape[1]).all()
            assert (np.diff(b[:, 0]) >= 0).all() and (np.diff(b[:, 0] + b[:, 1]) >= 0).all()      # the kernel's tiling relies on it
    assert preprocess.resample_tables(640, 512, "lanczos")[1] is preprocess.resample_tables(640, 512, "lanczos")[1]
    with pytest.raises(ValueError, match="unknown filter"):
        preprocess.resample_tables(640, 512, "bilinear")
    with pytest.raises(ValueError):
        preprocess.resample_tables(0, 512, "lanczos")


def test_overflow_check_raises_on_a_fabricated_table():
    ok = np.zeros((2, 5), np.int32)
    ok[:, 2] = 1 << 22
    preprocess.check_tables(ok)
    limit = ((1 << 31) - (1 << 21)) // 255                     # largest sum|k| is limit - 1 when 255 divides evenly
    edge = np.array([[(limit - 1) // 2, -((limit - 1) - (limit - 1) // 2), 0]], np.int32)
    assert int(np.abs(edge).sum()) == limit - 1
    assert 255 * int(np.abs(edge).sum()) + (1 << 21) < 1 << 31
    preprocess.check_tables(edge)
    bad = np.array([[limit // 2 + 1, -(limit // 2 + 1), 0]], np.int32)
    assert 255 * int(np.abs(bad).sum()) + (1 << 21) >= 1 << 31
    with pytest.raises(ValueError, match="overflow int32"):
        preprocess.check_tables(bad)
    with pytest.raises(ValueError, match="24-bit"):                         # the kernel multiplies with the 24-bit unit
        preprocess.check_tables(np.array([[1 << 23, 0, 0]], np.int32))
    preprocess.check_tables(np.array([[(1 << 23) - 1, 0, 0]], np.int32))


def _sweep_shapes():
    rng = np.random.default_rng(5)
    shapes = [(480, 640), (640, 480), (1080, 1920), (512, 512), (600, 600), (100, 100), (512, 384), (384, 512), (333, 517),
              (517, 333), (224, 224), (200, 224), (224, 300), (120, 160), (37, 100), (511, 512), (513, 512), (512, 300),
              (300, 512), (2160, 3840), (1000, 1000), (64, 4096), (4096, 64)]
    while len(shapes) < 230:
        shapes.append((int(rng.integers(20, 1400)), int(rng.integers(20, 1400))))
    return shapes


def test_resize_geometry_agrees_with_resize_img():
    checked = 0
    for h, w in _sweep_shapes():
        a = np.zeros((h, w, 3), np.uint8)
        for size in (512, 224):
            for square_ok in (False, True):
                try:
                    ref, tf = mast3r_utils.resize_img(a, size, square_ok=square_ok, return_transformation=True)
                except Exception:                                         # PIL refuses an empty result
                    with pytest.raises(ValueError):
                        preprocess.resize_geometry(h, w, size, square_ok)
                    continue
                if ref["unnormalized_img"].size == 0:
                    with pytest.raises(ValueError):
                        preprocess.resize_geometry(h, w, size, square_ok)
                    continue
                (W, H), kind, box, tf2 = preprocess.resize_geometry(h, w, size, square_ok)
                assert (box[3] - box[1], box[2] - box[0]) == ref["unnormalized_img"].shape[:2], (h, w, size, square_ok)
                assert ref["true_shape"].tolist() == [[box[3] - box[1], box[2] - box[0]]]
                assert tf2 == tf, (h, w, size, square_ok)
                assert 0 <= box[0] and box[2] <= W and 0 <= box[1] and box[3] <= H
                long_edge = round(size * max(w / h, h / w)) if size == 224 else size
                assert kind == ("lanczos" if max(h, w) > long_edge else "bicubic")
                assert twin.geometry(h, w, size, square_ok) == ((W, H), kind, box)
                checked += 1
    assert checked >= 800


@pytest.mark.parametrize("case", [((480, 640), 512, False), ((333, 517), 512, False), ((600, 600), 512, False),
                                  ((600, 600), 512, True), ((120, 160), 512, False), ((640, 480), 224, False),
                                  ((512, 384), 512, False), ((300, 700), 224, False)],
                         ids=lambda c: f"{c[0][1]}x{c[0][0]}-{c[1]}-{int(c[2])}")
def test_twin_resize_img_equals_resize_img(case):
    (h, w), size, square_ok = case
    a = make_content("noise", h, w, seed=h + w)
    ref = mast3r_utils.resize_img(a, size, square_ok=square_ok)
    raw, img = twin.resize_img(a, size, square_ok)
    assert raw.dtype == np.uint8 and np.array_equal(raw, ref["unnormalized_img"])
    assert img.dtype == np.float32 and np.array_equal(img.view(np.uint32), ref["img"].numpy().view(np.uint32))


def test_adjust_intrinsics_follows_a_projected_point():
    h1, w1 = 480, 640
    (W, H), _, box, tf = preprocess.resize_geometry(h1, w1, 224)
    assert box[0] > 0                                                     # a crop in x: both terms are exercised
    fx, fy, cx, cy = 525.0, 530.0, 319.5, 239.5
    P = np.array([0.3, -0.2, 2.0])
    u, v = fx * P[0] / P[2] + cx, fy * P[1] / P[2] + cy                   # pixel in the source image
    u2, v2 = u / tf[0] - tf[2], v / tf[1] - tf[3]                         # the same point after resize + crop
    k4 = preprocess.adjust_intrinsics([fx, fy, cx, cy], tf)
    assert np.allclose([k4[0] * P[0] / P[2] + k4[2], k4[1] * P[1] / P[2] + k4[3]], [u2, v2], atol=1e-9)
    K = torch.tensor([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=torch.float64)
    K2 = preprocess.adjust_intrinsics(K, tf)
    assert isinstance(K2, torch.Tensor) and K2.shape == (3, 3) and K[0, 0] == fx          # the input is not modified
    p = K2 @ torch.from_numpy(P)
    assert np.allclose((p[:2] / p[2]).numpy(), [u2, v2], atol=1e-9)
    assert K2[2].tolist() == [0, 0, 1]
    with pytest.raises(ValueError):
        preprocess.adjust_intrinsics(np.zeros(5), tf)


def test_device_path_refuses_cpu_and_non_uint8():
    with pytest.raises(RuntimeError, match="ROCm device"):
        preprocess.resize_img_device(torch.zeros((48, 64, 3), dtype=torch.uint8))
    with pytest.raises(TypeError):
        preprocess.resize_img_device(np.zeros((48, 64, 3), np.uint8))
    with pytest.raises(ValueError):
        preprocess.resize_img_device(torch.zeros((3, 48, 64), dtype=torch.uint8))
    for name in ("resize_img_device", "resize_geometry", "resample_tables", "adjust_intrinsics"):
        assert getattr(mast3r_utils, name) is getattr(preprocess, name) and name in mast3r_utils.__all__
    with pytest.raises(RuntimeError, match="ROCm device"):
        dataloader.ArrayDataset([np.zeros((48, 64, 3), np.uint8)]).frames("cpu").__next__()


def test_preprocess_symbol_is_declared_and_exported():
    assert "m3_resize_crop_u8" in _ffi.declared_symbols()
    L = _ffi.lib()
    assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), "m3_resize_crop_u8")
    assert L.m3_abi_version() == 4000
    # argument validation precedes every HIP call: safe without a device
    assert L.m3_resize_crop_u8(None, None, None, 1, None, None, 1, None, None, 1, 8, 8, 8, 8, 0, 0, 8, 8, None) == -1
    a16 = ctypes.c_void_p(4096)                                           # never dereferenced: the crop box is rejected first
    assert L.m3_resize_crop_u8(a16, None, None, 1, None, None, 1, a16, None, 1, 8, 8, 8, 8, 4, 0, 8, 8, None) == -1
    assert L.m3_resize_crop_u8(a16, None, None, 1, None, None, 1, a16, None, 1, 8, 8, 8, 4, 0, 0, 8, 4, None) == -1   # tables missing


# ---------------------------------------------------------------------------------------------------- dataset readers
def _png(path, value, hw=(6, 8)):
    from PIL import Image
    a = np.full(hw + (3,), value, np.uint8)
    a[0, 0] = (value, 0, 255 - value)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(a).save(path)


def test_config_has_the_reader_keys():
    ds = config.DEFAULT_CONFIG["dataset"]
    assert ds["subsample"] == 1 and ds["reverse"] is False


def test_folder_dataset(tmp_path):
    d = tmp_path / "seq"
    for i, name in enumerate(["b.png", "a.png", "c.PNG", "d.bmp", "notes.txt"]):
        if name.endswith(".txt"):
            (d / name).write_text("x")
        else:
            _png(str(d / name), 10 * (i + 1))
    ds = dataloader.load_dataset(d)
    assert isinstance(ds, dataloader.FolderDataset) and len(ds) == 4
    vals = [(t, int(f[1, 1, 0])) for t, f in ds]
    assert vals == [(0.0, 20), (1.0, 10), (2.0, 30), (3.0, 40)]                            # name order, timestamp = index
    t, f = ds[0]
    assert f.dtype == np.uint8 and f.shape == (6, 8, 3) and tuple(f[0, 0]) == (20, 0, 235)
    assert ds[-1][1][1, 1, 0] == 40
    with pytest.raises(IndexError):
        ds[4]
    config.set_config({"dataset": {"subsample": 2, "reverse": True}})
    try:
        ds = dataloader.load_dataset(str(d), "folder")
        assert [(t, int(f[1, 1, 0])) for t, f in ds] == [(0.0, 40), (1.0, 10)]             # reversed, then every second
    finally:
        config.reset_config()
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match="No images"):
        dataloader.load_dataset(tmp_path / "empty")
    with pytest.raises(ValueError, match="Unknown dataset type"):
        dataloader.load_dataset(d, "kitti")


def test_tum_dataset(tmp_path):
    d = tmp_path / "tum"
    for i, ts in enumerate(["1305031102.175304", "1305031102.211214", "1305031102.243211"]):
        _png(str(d / "rgb" / f"{ts}.png"), 50 + i)
    ds = dataloader.load_dataset(d)                                                        # rgb/ only: names are timestamps
    assert isinstance(ds, dataloader.TUMDataset) and len(ds) == 3
    assert [t for t, _ in ds] == [1305031102.175304, 1305031102.211214, 1305031102.243211]
    (d / "rgb.txt").write_text("# color images\n# timestamp filename\n"
                               "2.5 rgb/1305031102.243211.png\n1.5 rgb/1305031102.175304.png\n\nbroken\n")
    ds = dataloader.load_dataset(d)
    assert [(t, int(f[1, 1, 0])) for t, f in ds] == [(2.5, 52), (1.5, 50)]                 # file order, first column
    d2 = tmp_path / "tum2"
    _png(str(d2 / "images" / "x.png"), 7)
    (d2 / "associated.txt").write_text("0.25 images/x.png 0.26 depth/x.png\n")
    ds = dataloader.load_dataset(d2, "tum")
    assert len(ds) == 1 and ds[0][0] == 0.25 and ds[0][1][1, 1, 0] == 7
    (tmp_path / "tum3" / "rgb").mkdir(parents=True)
    with pytest.raises(ValueError, match="No frames"):
        dataloader.load_dataset(tmp_path / "tum3")


def test_euroc_dataset(tmp_path):
    for root, sub in (("e1", "mav0/cam0/data"), ("e2", "cam0/data")):
        for i, ns in enumerate(["1403636579763555584", "1403636579813555456"]):
            _png(str(tmp_path / root / sub / f"{ns}.png"), 90 + i)
        ds = dataloader.load_dataset(tmp_path / root)
        assert isinstance(ds, dataloader.EuRoCDataset) and len(ds) == 2
        assert [t for t, _ in ds] == [1403636579763555584 / 1e9, 1403636579813555456 / 1e9]
        assert ds[1][1][1, 1, 0] == 91
    (tmp_path / "e3" / "mav0").mkdir(parents=True)
    with pytest.raises(ValueError, match="Camera directory"):
        dataloader.load_dataset(tmp_path / "e3")


def test_video_dataset_needs_cv2(tmp_path):
    try:
        import cv2  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="cv2"):
            dataloader.load_dataset(tmp_path / "clip.mp4")
    else:
        with pytest.raises(ValueError, match="Could not open"):
            dataloader.load_dataset(tmp_path / "clip.mp4")


def test_array_dataset():
    frames = [np.full((4, 6, 3), i, np.uint8) for i in range(5)]
    ds = dataloader.ArrayDataset(frames)
    assert len(ds) == 5 and [t for t, _ in ds] == [0.0, 1.0, 2.0, 3.0, 4.0] and ds[3][1][0, 0, 0] == 3
    ds = dataloader.ArrayDataset(frames, timestamps=[0.5, 0.6, 0.7, 0.8, 0.9])
    assert ds[2][0] == 0.7 and isinstance(ds[2][1], np.ndarray)
    with pytest.raises(ValueError):
        dataloader.ArrayDataset(frames, timestamps=[1.0])
    with pytest.raises(ValueError):
        dataloader.ArrayDataset([])
    config.set_config({"dataset": {"subsample": 2}})
    try:
        assert [int(f[0, 0, 0]) for _, f in dataloader.ArrayDataset(frames)] == [0, 2]
    finally:
        config.reset_config()
