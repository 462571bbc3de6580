"""Host: the camera model, the undistortion table and the calibration readers of mast3r_slam/camera.py, and
tests/undistort_twin.py against the MEANING of the model: a smooth image seen through the lens and remapped by the twin
comes back where the ideal camera sees it (a device-equals-twin test cannot see a map applied in the wrong direction)."""
import json
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import undistort_twin as twin  # noqa: E402

from mast3r_slam import camera, config, dataloader, mast3r_utils, preprocess  # noqa: E402
from mast3r_slam.camera import CameraModel  # noqa: E402

CAMS = {
    "euroc": dict(width=752, height=480, K=[458.654, 457.296, 367.215, 248.375],
                  distortion=(-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05), model="radtan"),
    "tum1": dict(width=640, height=480, K=[517.3, 516.5, 318.6, 255.3],
                 distortion=(0.2624, -0.9531, -0.0054, 0.0026, 1.1633), model="radtan"),
    "small": dict(width=61, height=45, K=[48, 47, 30.2, 21.7], distortion=(-0.25, 0.06, 0.001, -0.002), model="radtan"),
}
EQUI = dict(width=640, height=480, K=[380.0, 381.0, 322.5, 236.0], distortion=(0.03, -0.02, 0.01, -0.005), model="equidistant")
INNER = {"euroc": [356.017, 418.236, 362.992, 250.272], "tum1": [546.636, 543.009, 320.076, 251.882]}


def _cam(name):
    return CameraModel(**CAMS[name])


def _pixel_centres(c):
    """Normalised (distorted) coordinates of every pixel centre, [H, W, 2]."""
    fx, fy, cx, cy = c["K"]
    u, v = np.meshgrid(np.arange(c["width"], dtype=np.float64), np.arange(c["height"], dtype=np.float64))
    return np.stack([(u - cx) / fx, (v - cy) / fy], -1)


@pytest.mark.parametrize("spec", list(CAMS.values()) + [EQUI], ids=list(CAMS) + ["equidistant"])
def test_distort_inverts_undistort_at_every_pixel_centre(spec):
    cam = CameraModel(**spec)
    p = _pixel_centres(spec)
    ideal = cam.undistort_points(p)
    assert ideal.shape == p.shape and np.isfinite(ideal).all()
    xd, yd = twin.distort(spec["model"], spec["distortion"], ideal[..., 0], ideal[..., 1])     # the twin's forward model
    err = max(np.abs(xd - p[..., 0]).max(), np.abs(yd - p[..., 1]).max())
    print(f"max |distort(undistort(p)) - p| = {err:.3g}")
    assert err < 1e-10
    assert np.abs(cam.distort_points(ideal) - np.stack([xd, yd], -1)).max() < 1e-14              # two statements, one model


def test_forward_models_at_hand_computed_points():
    cam = CameraModel(100, 100, [50, 50, 50, 50], (0.1, 0.01, 0.002, -0.003, 0.001), "radtan")
    x, y = 0.5, -0.25
    r2 = x * x + y * y
    rad = 1 + 0.1 * r2 + 0.01 * r2 ** 2 + 0.001 * r2 ** 3
    want = (x * rad + 2 * 0.002 * x * y - 0.003 * (r2 + 2 * x * x), y * rad + 0.002 * (r2 + 2 * y * y) + 2 * -0.003 * x * y)
    assert np.allclose(cam.distort_points([x, y]), want, rtol=0, atol=1e-15)
    eq = CameraModel(100, 100, [50, 50, 50, 50], (0.03, -0.02, 0.01, -0.005), "equidistant")
    r = np.hypot(x, y)
    th = np.arctan(r)
    thd = th * (1 + 0.03 * th ** 2 - 0.02 * th ** 4 + 0.01 * th ** 6 - 0.005 * th ** 8)
    assert np.allclose(eq.distort_points([x, y]), (x * thd / r, y * thd / r), rtol=0, atol=1e-15)
    assert np.array_equal(eq.distort_points([[0.0, 0.0]]), [[0.0, 0.0]])
    # a missing k3 is 0; pinhole or all-zero coefficients are no distortion
    assert CameraModel(10, 10, [5, 5, 5, 5], (0.1, 0.2, 0.3, 0.4), "radtan").distortion == (0.1, 0.2, 0.3, 0.4, 0.0)
    assert not CameraModel(10, 10, [5, 5, 5, 5]).has_distortion
    assert not CameraModel(10, 10, [5, 5, 5, 5], (0, 0, 0, 0), "radtan").has_distortion
    assert cam.has_distortion and eq.has_distortion
    for bad in (dict(distortion=(0.1,), model="radtan"), dict(distortion=(0.1,) * 5, model="equidistant"),
                dict(distortion=(0.1,), model="pinhole"), dict(model="fisheye62")):
        with pytest.raises(ValueError):
            CameraModel(10, 10, [5, 5, 5, 5], **bad)


def test_an_inverse_that_cannot_converge_raises_or_is_nan():
    # th < pi / 2, so the distorted radius th (1 + 0.01 th^2) stays below 1.61: the point (5, 0) has no preimage
    cam = CameraModel(100, 100, [50, 50, 50, 50], (0.01, 0, 0, 0), "equidistant")
    with pytest.raises(ValueError, match="no inverse"):
        cam.undistort_points([[0.1, 0.0], [5.0, 0.0]])
    out = cam.undistort_points([[0.1, 0.0], [5.0, 0.0]], strict=False)
    assert np.isfinite(out[0]).all() and np.isnan(out[1]).all()
    assert np.abs(cam.distort_points(out[0]) - [0.1, 0.0]).max() < 1e-10
    wide = CameraModel(2000, 100, [50, 50, 1000, 50], (0.01, 0, 0, 0), "equidistant")  # its border has no inverse
    with pytest.raises(ValueError):
        wide.new_camera_matrix("inner")


@pytest.mark.parametrize("name", list(CAMS))
@pytest.mark.parametrize("mode", ("same", "inner"))
def test_table_entries_mean_the_source_coordinate(name, mode):
    c, cam = CAMS[name], _cam(name)
    tab = cam.undistort_table(mode)
    assert tab.dtype == np.int32 and tab.shape == (c["height"], c["width"], 2) and not tab.flags.writeable
    assert cam.undistort_table(mode) is tab                                            # cached
    K_new = cam.new_camera_matrix(mode)
    if mode == "same":
        assert list(K_new) == [float(v) for v in c["K"]]
    sx, sy = twin.source_coords(c["model"], c["K"], c["distortion"], K_new, (c["width"], c["height"]))
    keep = (tab != twin.SENTINEL).all(-1)
    assert keep.mean() > 0.99
    bound = 0.5 / 256 + 1e-6                                                           # rounding + float64 slack
    assert np.abs(tab[..., 0] / 256.0 - sx)[keep].max() <= bound
    assert np.abs(tab[..., 1] / 256.0 - sy)[keep].max() <= bound
    assert np.array_equal(tab, twin.table(c["model"], c["K"], c["distortion"], K_new, (c["width"], c["height"])))


def test_table_default_out_size_sentinels_and_explicit_matrix():
    cam = _cam("small")
    assert cam.undistort_table() is cam.undistort_table("inner")                       # the default K_new
    t = cam.undistort_table([40.0, 41.0, 18.0, 14.0], out_size=(37, 29))
    assert t.shape == (29, 37, 2)
    assert np.array_equal(t, twin.table("radtan", CAMS["small"]["K"], CAMS["small"]["distortion"], [40.0, 41.0, 18.0, 14.0], (37, 29)))
    # a field of view so wide that the polynomial leaves 2^20 pixels: sentinels, and only there
    far = CameraModel(64, 48, [48, 47, 30.2, 21.7], (0.2, 0.3, 0.0, 0.0, 0.9), "radtan")
    tf = far.undistort_table([0.05, 0.05, 32.0, 24.0])
    sx, sy = twin.source_coords("radtan", far.K, far.distortion, [0.05, 0.05, 32.0, 24.0], (64, 48))
    sent = (tf == twin.SENTINEL).all(-1)
    assert sent.any() and not sent.all()
    assert np.array_equal(sent, ~((np.abs(sx) < 2 ** 20) & (np.abs(sy) < 2 ** 20)))
    with pytest.raises(ValueError):
        cam.undistort_table("outer")


@pytest.mark.parametrize("name", list(CAMS))
def test_inner_matrix_is_valid_and_tight(name):
    c, cam = CAMS[name], _cam(name)
    W, H = c["width"], c["height"]
    K_new = cam.new_camera_matrix("inner")
    if name in INNER:
        assert np.abs(np.array(K_new) - INNER[name]).max() < 1e-3, K_new
    tab = cam.undistort_table("inner").astype(np.int64)
    assert not (tab == twin.SENTINEL).any()
    ix, iy, a, b = tab[..., 0] >> 8, tab[..., 1] >> 8, tab[..., 0] & 255, tab[..., 1] & 255
    # every tap with a non-zero weight is inside the source
    assert ix.min() >= 0 and iy.min() >= 0
    assert (ix + (a > 0)).max() <= W - 1 and (iy + (b > 0)).max() <= H - 1
    # each side of the output touches that side of the source somewhere, within a pixel
    sx, sy = twin.source_coords(c["model"], c["K"], c["distortion"], K_new, (W, H))
    gaps = {"left": np.abs(sx[:, 0]).min(), "right": np.abs(sx[:, -1] - (W - 1)).min(),
            "top": np.abs(sy[0]).min(), "bottom": np.abs(sy[-1] - (H - 1)).min()}
    print(name, {k: round(float(v), 4) for k, v in gaps.items()}, "raw coordinates leave the source by",
          max(-sx.min(), -sy.min(), sx.max() - (W - 1), sy.max() - (H - 1)))
    assert max(gaps.values()) < 1.0, gaps
    if name in ("euroc", "small"):
        # A barrel lens: the border pixel that sets a side of the rectangle lies inside that side, where the side's source
        # coordinate is stationary along it.  The nearest output pixel is at most half a step from that point, so its
        # gap is at most M2 / 8, M2 = the largest second difference of the coordinate along the side (+ float64 slack).
        m2 = {"left": np.abs(np.diff(sx[:, 0], 2)).max(), "right": np.abs(np.diff(sx[:, -1], 2)).max(),
              "top": np.abs(np.diff(sy[0], 2)).max(), "bottom": np.abs(np.diff(sy[-1], 2)).max()}
        for side, gap in gaps.items():
            print(name, side, "gap", float(gap), "bound", float(m2[side] / 8 + 1e-6))
            assert gap <= m2[side] / 8 + 1e-6, (side, gap, m2[side] / 8)


def test_inner_of_an_undistorted_camera_is_its_own_matrix():
    cam = CameraModel(64, 48, [50.0, 51.0, 31.5, 23.5], (0, 0, 0, 0), "radtan")
    assert cam.new_camera_matrix("inner") == cam.K == cam.new_camera_matrix("same")
    tab = cam.undistort_table()
    u, v = np.meshgrid(np.arange(64), np.arange(48))
    assert np.array_equal(tab[..., 0], u << 8) and np.array_equal(tab[..., 1], v << 8)


# ---------------------------------------------------------------------- the twin against the meaning of the model
WAVES = ((9.0, 4.0, 0.3), (3.0, -11.0, 1.0), (-6.0, 7.0, 2.0))


def _ideal_image(x, y):
    return np.stack([127.5 + 100.0 * np.sin(al * x + be * y + ph) for al, be, ph in WAVES], -1)


@pytest.mark.parametrize("scale", (0.25, 1.0), ids=("160x120", "640x480"))
def test_twin_remap_returns_the_ideal_image(scale):
    """The distorted source is the smooth image I_c(x, y) = 127.5 + 100 sin(al x + be y + ph) over ideal coordinates,
    sampled where each source pixel really looks (undistort_points) and rounded to uint8; the twin's remap with
    K_new = "same" must give I_c at the ideal coordinates of the output pixels.  Bound, in grey levels, from
      0.5 source rounding (bilinear weights are convex) + 0.5 output rounding
      + (M2x + M2y) / 8 bilinear interpolation, M2 = largest second derivative of the unrounded source, per source pixel
      + (|dI/dsx| + |dI/dsy|) / 512 for the 1/256-pixel quantisation of each source coordinate,
    the derivatives being centred differences of the unrounded source image (the waves span > 70 pixels at the small
    size).  About 1.15 at 160x120.  Measured on the CPU: 1.010 at 160x120, 0.972 at 640x480; 0.933 / 0.940 of the
    pixels have their four taps inside and are compared."""
    c = CAMS["tum1"]
    W, H = int(c["width"] * scale), int(c["height"] * scale)
    K = [v * scale for v in c["K"]]
    cam = CameraModel(W, H, K, c["distortion"], c["model"])
    spec = dict(width=W, height=H, K=K)
    ideal = cam.undistort_points(_pixel_centres(spec))
    S = _ideal_image(ideal[..., 0], ideal[..., 1])                                     # float source, [H, W, 3]
    src = np.floor(S + 0.5).astype(np.uint8)
    tab = twin.table(c["model"], K, c["distortion"], K, (W, H))
    out = twin.remap(src, tab).astype(np.float64)
    p = _pixel_centres(spec)
    want = _ideal_image(p[..., 0], p[..., 1])
    inside = twin.taps_inside(tab, H, W)
    share = inside.mean()
    m2x = np.abs(S[:, 2:] - 2 * S[:, 1:-1] + S[:, :-2]).max(axis=(0, 1))
    m2y = np.abs(S[2:] - 2 * S[1:-1] + S[:-2]).max(axis=(0, 1))
    gx = np.abs(S[:, 2:] - S[:, :-2]).max(axis=(0, 1)) / 2
    gy = np.abs(S[2:] - S[:-2]).max(axis=(0, 1)) / 2
    bound = float((0.5 + 0.5 + (m2x + m2y) / 8 + (gx + gy) / 512).max())
    err = float(np.abs(out - want)[inside].max())
    print(f"{W}x{H}: max error {err:.3f} grey levels, bound {bound:.3f}, share compared {share:.3f}")
    assert share >= 0.9
    assert err <= bound
    # the map applied the wrong way round (the source looked up at the undistorted position) is far outside the bound
    wrong = np.stack([np.floor((ideal[..., 0] * K[0] + K[2]) * 256 + 0.5), np.floor((ideal[..., 1] * K[1] + K[3]) * 256 + 0.5)], -1)
    bad = twin.remap(src, wrong.astype(np.int32)).astype(np.float64)
    assert np.abs(bad - want)[inside & twin.taps_inside(wrong.astype(np.int32), H, W)].max() > 10 * bound


# ---------------------------------------------------------------------- calibration files and datasets
def _write(path, text):
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(text)
    return path


SENSOR_YAML = """# General sensor definitions.
sensor_type: camera
comment: VI-Sensor cam0 (MT9M034)
T_BS:
  cols: 4
  rows: 4
  data: [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]
rate_hz: 20
resolution: [752, 480]
camera_model: pinhole
intrinsics: [458.654, 457.296, 367.215, 248.375] #fu, fv, cu, cv
distortion_model: radial-tangential
distortion_coefficients: [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05]
"""


def test_load_calibration_three_forms(tmp_path):
    euroc = _cam("euroc")
    assert camera.load_calibration(_write(tmp_path / "sensor.yaml", SENSOR_YAML)) == euroc
    own = {"width": 752, "height": 480, "model": "radtan", "intrinsics": CAMS["euroc"]["K"],
           "distortion": list(CAMS["euroc"]["distortion"])}
    assert camera.load_calibration(own) == euroc
    assert camera.load_calibration(_write(tmp_path / "c.json", json.dumps(own))) == euroc
    assert camera.load_calibration(_write(tmp_path / "c.yaml", "width: 752\nheight: 480\nmodel: radtan\n"
                                          f"intrinsics: {CAMS['euroc']['K']}\ndistortion: {list(CAMS['euroc']['distortion'])}\n")) == euroc
    flat = {"width": 640, "height": 480, "calibration": CAMS["tum1"]["K"] + list(CAMS["tum1"]["distortion"])}
    assert camera.load_calibration(flat) == _cam("tum1")
    assert camera.load_calibration(_write(tmp_path / "flat.yaml", f"width: 640\nheight: 480\ncalibration: {flat['calibration']}\n")) == _cam("tum1")
    four = camera.load_calibration({"width": 640, "height": 480, "calibration": [500, 501, 320, 240]})
    assert four.model == "pinhole" and not four.has_distortion and four.K == (500.0, 501.0, 320.0, 240.0)
    eq = camera.load_calibration(_write(tmp_path / "eq.yaml", SENSOR_YAML.replace("radial-tangential", "equidistant")))
    assert eq.model == "equidistant" and eq.distortion == CAMS["euroc"]["distortion"]
    assert camera.load_calibration(euroc) is euroc
    assert mast3r_utils.load_calibration is camera.load_calibration and mast3r_utils.CameraModel is CameraModel
    assert mast3r_utils.undistort_device is camera.undistort_device


def test_load_calibration_errors_name_the_file(tmp_path):
    p = _write(tmp_path / "sensor.yaml", SENSOR_YAML.replace("radial-tangential", "fov"))
    with pytest.raises(ValueError, match="sensor.yaml.*fov"):
        camera.load_calibration(p)
    p = _write(tmp_path / "short.yaml", SENSOR_YAML.replace("0.00019359, 1.76187114e-05", "0.00019359"))
    with pytest.raises(ValueError, match="short.yaml"):
        camera.load_calibration(p)
    p = _write(tmp_path / "flat.yaml", "width: 640\nheight: 480\ncalibration: [500, 500, 320, 240, 0.1]\n")
    with pytest.raises(ValueError, match="flat.yaml"):
        camera.load_calibration(p)
    p = _write(tmp_path / "own.json", json.dumps({"width": 4, "height": 4, "model": "kannala", "intrinsics": [1, 1, 1, 1]}))
    with pytest.raises(ValueError, match="own.json.*kannala"):
        camera.load_calibration(p)
    p = _write(tmp_path / "nosize.yaml", "intrinsics: [1, 1, 1, 1]\n")
    with pytest.raises(ValueError, match="nosize.yaml"):
        camera.load_calibration(p)
    with pytest.raises(ValueError, match="broken.yaml"):
        camera.load_calibration(_write(tmp_path / "broken.yaml", "width: [1, 2\n"))


def _png(path, h=45, w=61):
    from PIL import Image
    path.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(np.zeros((h, w, 3), np.uint8)).save(path)


OWN_YAML = "width: 61\nheight: 45\nmodel: radtan\nintrinsics: [48, 47, 30.2, 21.7]\ndistortion: [-0.25, 0.06, 0.001, -0.002]\n"


def test_readers_pick_up_their_calibration(tmp_path):
    e = tmp_path / "euroc"
    _png(e / "mav0" / "cam0" / "data" / "1403636579763555584.png")
    assert dataloader.load_dataset(e).calibration is None
    _write(e / "mav0" / "cam0" / "sensor.yaml", SENSOR_YAML)
    ds = dataloader.load_dataset(e)
    assert isinstance(ds, dataloader.EuRoCDataset) and ds.calibration == _cam("euroc")
    _write(e / "calibration.yaml", OWN_YAML)                                # the project's own file wins
    assert dataloader.load_dataset(e).calibration == _cam("small")
    f = tmp_path / "folder"
    _png(f / "000.png")
    assert dataloader.load_dataset(f).calibration is None
    _write(f / "calibration.json", json.dumps({"width": 61, "height": 45, "calibration": [48, 47, 30.2, 21.7, -0.25, 0.06, 0.001, -0.002]}))
    assert dataloader.load_dataset(f).calibration == _cam("small")
    t = tmp_path / "tum"
    _png(t / "rgb" / "1.5.png")
    _write(t / "calibration.yaml", OWN_YAML)
    assert isinstance(dataloader.load_dataset(t), dataloader.TUMDataset) and dataloader.load_dataset(t).calibration == _cam("small")
    # an explicit calibration replaces what the reader found: a CameraModel, a path or a mapping
    assert dataloader.load_dataset(t, calibration=_cam("tum1")).calibration == _cam("tum1")
    assert dataloader.load_dataset(f, calibration=e / "mav0" / "cam0" / "sensor.yaml").calibration == _cam("euroc")
    assert dataloader.load_dataset(f, calibration={"width": 8, "height": 8, "calibration": [4, 4, 4, 4]}).calibration.K == (4.0,) * 4
    assert dataloader.ArrayDataset([np.zeros((45, 61, 3), np.uint8)]).calibration is None


def test_an_explicit_calibration_keeps_a_broken_file_beside_the_frames_closed(tmp_path):
    f = tmp_path / "folder"
    _png(f / "000.png")
    _write(f / "calibration.yaml", "width: 61\nheight: 45\nmodel: fisheye9\nintrinsics: [1, 2, 3, 4]\n")
    with pytest.raises(ValueError, match="calibration.yaml"):
        dataloader.load_dataset(f)
    assert dataloader.load_dataset(f, calibration=_cam("small")).calibration == _cam("small")
    assert dataloader.FolderDataset(f, calibration=_cam("tum1")).calibration == _cam("tum1")
    e = tmp_path / "euroc"
    _png(e / "mav0" / "cam0" / "data" / "1403636579763555584.png")
    _write(e / "mav0" / "cam0" / "sensor.yaml", "resolution: [752]\n")
    with pytest.raises(ValueError, match="sensor.yaml"):
        dataloader.load_dataset(e)
    assert dataloader.load_dataset(e, calibration=_cam("euroc")).calibration == _cam("euroc")


def test_dataset_intrinsics_is_the_adjust_intrinsics_composition():
    frames = [np.zeros((480, 640, 3), np.uint8)]
    cam = _cam("tum1")
    ds = dataloader.ArrayDataset(frames, calibration=cam)
    assert dataloader.ArrayDataset(frames).intrinsics(512) is None
    for size, square_ok in ((512, False), (224, False), (512, True)):
        want = preprocess.adjust_intrinsics(np.array(cam.new_camera_matrix("inner")), preprocess.resize_geometry(480, 640, size, square_ok)[3])
        got = ds.intrinsics(size, square_ok)
        assert got.shape == (4,) and np.array_equal(got, want)
    assert np.array_equal(ds.intrinsics(), ds.intrinsics(config.get_config()["dataset"]["img_size"]))
    config.set_config({"dataset": {"new_camera_matrix": "same"}})
    try:
        want = preprocess.adjust_intrinsics(np.array(cam.K), preprocess.resize_geometry(480, 640, 512)[3])
        assert np.array_equal(ds.intrinsics(512), want)
    finally:
        config.reset_config()
    assert "new_camera_matrix" not in config.get_config()["dataset"] and "undistort" not in config.get_config()["dataset"]


def test_run_dataset_refuses_two_sources_of_intrinsics():
    import torch

    from mast3r_slam.slam import SLAM
    model = types.SimpleNamespace(device=torch.device("cpu"))                # the error comes before any device use
    ds = dataloader.ArrayDataset([np.zeros((480, 640, 3), np.uint8)], calibration=_cam("tum1"))
    s = SLAM(model, K=torch.tensor([[525.0, 0, 319.5], [0, 525.0, 239.5], [0, 0, 1]]))
    with pytest.raises(ValueError, match=r"(?s)K.*calibration"):
        s.run_dataset(ds)
    assert len(s.keyframes) == 0


def test_device_entry_points_refuse_the_host():
    import torch
    cam = _cam("small")
    with pytest.raises(RuntimeError, match="no CPU path"):
        camera.undistort_device(torch.zeros((45, 61, 3), dtype=torch.uint8), cam)
    ds = dataloader.ArrayDataset([np.zeros((45, 61, 3), np.uint8)], calibration=cam)
    with pytest.raises(RuntimeError):
        next(iter(ds.frames("cpu")))
    with pytest.raises(ValueError, match="needs a calibration"):
        next(iter(dataloader.ArrayDataset([np.zeros((45, 61, 3), np.uint8)]).frames("cuda", undistort=True)))


def test_library_exports_the_remap_and_checks_its_arguments_on_the_host():
    import ctypes

    from mast3r_slam import _ffi
    assert "m3_remap_bilinear_u8" in _ffi.declared_symbols()
    L = _ffi.lib()
    assert L.m3_abi_version() == 4000                                        # a symbol was added, nothing changed
    a = ctypes.c_void_p(4096)                                                # never dereferenced: every call is refused first
    f = L.m3_remap_bilinear_u8
    assert f(None, a, a, 1, 4, 4, 4, 4, 0, None) == -1 and f(a, None, a, 1, 4, 4, 4, 4, 0, None) == -1
    assert f(a, a, None, 1, 4, 4, 4, 4, 0, None) == -1
    assert f(ctypes.c_void_p(4100), a, a, 1, 4, 4, 4, 4, 0, None) == -1       # misaligned
    assert f(a, ctypes.c_void_p(4104), a, 1, 4, 4, 4, 4, 0, None) == -1
    for bad in ((0, 4, 4, 4, 4, 0), (65536, 4, 4, 4, 4, 0), (1, 0, 4, 4, 4, 0), (1, 4, -1, 4, 4, 0), (1, 4, 4, 0, 4, 0),
                (1, 4, 4, 4, 0, 0), (1, 4, 4, 4, 4, 256), (1, 4, 4, 4, 4, -1), (1, (1 << 20) + 1, 4, 4, 4, 0)):
        assert f(a, a, a, *bad, None) == -1, bad
