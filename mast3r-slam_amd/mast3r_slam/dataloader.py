"""Dataset readers (the behaviour of the reference's dataloader.py:37-268: folder, TUM, EuRoC, video, load_dataset) and
the step from a camera-sized frame to a network-sized one on the device (Dataset.frames over
preprocess.resize_img_device).  Decoding stays on the host (PIL / cv2); undistortion (mast3r_slam/camera.py), resizing and cropping do not.

A dataset is a sequence of (timestamp, uint8 [H,W,3] numpy RGB).  `dataset.subsample` / `dataset.reverse` of the
config are read when a reader is built, as in the reference.
"""
from __future__ import annotations

import os
from pathlib import Path
from typing import Iterator, Optional, Sequence

import numpy as np
import torch

from .camera import CameraModel, find_calibration, load_calibration, undistort_device
from .config import get_config
from .preprocess import adjust_intrinsics, resize_geometry, resize_img_device

IMAGE_EXTENSIONS = (".jpg", ".jpeg", ".png", ".bmp")
VIDEO_EXTENSIONS = (".mp4", ".avi", ".mov", ".mkv")


def _read_rgb(path) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"))


class Dataset:
    """len / getitem -> (timestamp, uint8 [H,W,3]) / iter.  Readers fill `self._entries` with what `_load` takes, in
    time order; subsample and reverse are applied here."""

    def __init__(self) -> None:
        ds = get_config()["dataset"]
        self.subsample = max(int(ds.get("subsample", 1)), 1)
        self.reverse = bool(ds.get("reverse", False))
        self._entries: list = []
        self.calibration: Optional[CameraModel] = None     # readers pick up a calibration file; load_dataset may set one

    def _pick_calibration(self, explicit, *candidates) -> None:
        """`explicit` (a CameraModel, file or mapping) if given; else the first of `candidates` (directories searched for
        calibration.yaml / .json, or calibration files) that exists.  With an explicit calibration no file beside the
        frames is opened, so a broken one there cannot get in the way."""
        if explicit is not None:
            self.calibration = load_calibration(explicit)
            return
        for c in candidates:
            c = Path(c)
            cam = find_calibration(c) if c.is_dir() else (load_calibration(c) if c.is_file() else None)
            if cam is not None:
                self.calibration = cam
                return

    def _new_camera_matrix(self):
        """config["dataset"]["new_camera_matrix"] (optional: "inner", "same" or [fx, fy, cx, cy]) of the undistorted frames."""
        return get_config()["dataset"].get("new_camera_matrix", "inner")

    def intrinsics(self, size: Optional[int] = None, square_ok: bool = False):
        """[fx, fy, cx, cy] (float64 array) of the frames that `frames` yields for a calibrated dataset: the undistorted
        camera moved through the resize and crop; None without a calibration."""
        cam = self.calibration
        if cam is None:
            return None
        if size is None:
            size = get_config()["dataset"]["img_size"]
        K_new = np.array(cam.new_camera_matrix(self._new_camera_matrix()), dtype=np.float64)
        return adjust_intrinsics(K_new, resize_geometry(cam.height, cam.width, size, square_ok)[3])

    def _finish(self, what: str) -> None:
        if not self._entries:
            raise ValueError(what)
        if self.reverse:
            self._entries = self._entries[::-1]

    def _load(self, entry, idx: int):
        raise NotImplementedError

    def __len__(self) -> int:
        return len(self._entries) // self.subsample

    def __getitem__(self, idx: int):
        n = len(self)
        if idx < 0:
            idx += n
        if not 0 <= idx < n:
            raise IndexError(f"index {idx} out of range for {n} frames")
        return self._load(self._entries[idx * self.subsample], idx)

    def __iter__(self) -> Iterator:
        for i in range(len(self)):
            yield self[i]

    # ------------------------------------------------------------------ device preprocessing
    def frames(self, device, size: Optional[int] = None, square_ok: bool = False, batch: int = 1,
               undistort: Optional[bool] = None):
        """Generator of (timestamp, uint8 [H',W',3] on `device`): each raw frame is uploaded as it was decoded and
        resized + cropped there (resize_img_device).  `batch` frames share one upload and one launch while their
        source shapes agree.  size None: config["dataset"]["img_size"].  This is what SLAM.run takes.
        With a calibration the uploaded batch is undistorted first (camera.undistort_device: a second launch) and
        `intrinsics` describes the result; undistort=False skips it, None reads the optional
        config["dataset"]["undistort"] (default True).  A frame of another size than the calibration's raises."""
        if size is None:
            size = get_config()["dataset"]["img_size"]
        if undistort is None:
            undistort = self.calibration is not None and bool(get_config()["dataset"].get("undistort", True))
        elif undistort and self.calibration is None:
            raise ValueError("frames: undistort=True needs a calibration (Dataset.calibration is None)")
        cam, K_new = (self.calibration, self._new_camera_matrix()) if undistort else (None, None)
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"frames: must target the ROCm device (got {device}); no CPU path exists")
        batch = max(int(batch), 1)
        pending: list = []

        def flush():
            raw = np.stack([f for _, f in pending]) if len(pending) > 1 else pending[0][1][None]
            src = torch.from_numpy(np.ascontiguousarray(raw)).to(device)
            if cam is not None:
                src = undistort_device(src, cam, K_new)
            out = resize_img_device(src, size, square_ok)
            imgs = out["unnormalized_img"]
            res = [(t, imgs[i]) for i, (t, _) in enumerate(pending)]
            pending.clear()
            return res

        for t, frame in self:
            frame = np.asarray(frame)
            if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
                raise TypeError(f"frames: expected uint8 [H,W,3], got {frame.dtype} {frame.shape}")
            if pending and pending[0][1].shape != frame.shape:
                yield from flush()
            pending.append((t, frame))
            if len(pending) == batch:
                yield from flush()
        if pending:
            yield from flush()


class ArrayDataset(Dataset):
    """Frames already in memory (a decoded video, a camera, a test): a sequence of uint8 [H,W,3] arrays."""

    def __init__(self, frames: Sequence, timestamps: Optional[Sequence[float]] = None, calibration=None) -> None:
        super().__init__()
        if calibration is not None:
            self.calibration = load_calibration(calibration)
        if timestamps is not None and len(timestamps) != len(frames):
            raise ValueError(f"{len(frames)} frames but {len(timestamps)} timestamps")
        ts = [float(t) for t in timestamps] if timestamps is not None else [float(i) for i in range(len(frames))]
        self._entries = list(zip(ts, frames))
        self._finish("ArrayDataset needs at least one frame")

    def _load(self, entry, idx):
        t, f = entry
        return t, np.asarray(f.cpu() if isinstance(f, torch.Tensor) else f)


class FolderDataset(Dataset):
    """A folder of images in name order; the timestamp of a frame is its index."""

    def __init__(self, path, extensions: Sequence[str] = IMAGE_EXTENSIONS, calibration=None) -> None:
        super().__init__()
        self.path = Path(path)
        self.extensions = tuple(extensions)
        self._entries = sorted(f for f in self.path.iterdir() if f.suffix.lower() in self.extensions)
        self._finish(f"No images found in {path} with extensions {self.extensions}")
        self._pick_calibration(calibration, self.path)
        self.images = self._entries

    def _load(self, entry, idx):
        return float(idx), _read_rgb(entry)


class TUMDataset(Dataset):
    """TUM RGB-D layout: rgb.txt (or associated.txt) lines "timestamp path", `#` lines skipped; without either file
    the rgb/*.png files, whose names are the timestamps."""

    def __init__(self, path, calibration=None) -> None:
        super().__init__()
        self.path = Path(path)
        listing = self.path / "rgb.txt"
        if not listing.exists():
            listing = self.path / "associated.txt"
        if listing.exists():
            with open(listing) as f:
                for line in f:
                    if line.startswith("#"):
                        continue
                    parts = line.split()
                    if len(parts) >= 2:
                        self._entries.append((float(parts[0]), self.path / parts[1]))
        elif (self.path / "rgb").exists():
            self._entries = [(float(p.stem), p) for p in sorted((self.path / "rgb").glob("*.png"))]
        self._finish(f"No frames found in TUM dataset at {path}")
        self._pick_calibration(calibration, self.path)

    def _load(self, entry, idx):
        return entry[0], _read_rgb(entry[1])


class EuRoCDataset(Dataset):
    """EuRoC MAV layout: mav0/cam0/data/*.png (or cam0/data), file names are nanosecond timestamps.  The camera's
    sensor.yaml beside data/ is the calibration unless the dataset directory holds a calibration.yaml / .json."""

    def __init__(self, path, calibration=None) -> None:
        super().__init__()
        self.path = Path(path)
        cam = self.path / "mav0" / "cam0" / "data"
        if not cam.exists():
            cam = self.path / "cam0" / "data"
        if not cam.exists():
            raise ValueError(f"Camera directory not found in EuRoC dataset at {path}")
        self._entries = [(float(p.stem) / 1e9, p) for p in sorted(cam.glob("*.png"))]
        self._finish(f"No frames found in EuRoC dataset at {path}")
        self._pick_calibration(calibration, self.path, cam.parent / "sensor.yaml")

    def _load(self, entry, idx):
        return entry[0], _read_rgb(entry[1])


class VideoDataset(Dataset):
    """A video file decoded by OpenCV; timestamp = frame number / fps."""

    def __init__(self, path, calibration=None) -> None:
        super().__init__()
        try:
            import cv2
        except ImportError:
            raise ImportError("OpenCV (cv2) required for video datasets")
        self.path = Path(path)
        self.cap = cv2.VideoCapture(str(self.path))
        if not self.cap.isOpened():
            raise ValueError(f"Could not open video: {path}")
        self.fps = self.cap.get(cv2.CAP_PROP_FPS)
        self._entries = list(range(int(self.cap.get(cv2.CAP_PROP_FRAME_COUNT))))
        self._finish(f"No frames found in video {path}")
        self._pick_calibration(calibration, self.path.parent)

    def _load(self, entry, idx):
        import cv2
        self.cap.set(cv2.CAP_PROP_POS_FRAMES, entry)
        ok, frame = self.cap.read()
        if not ok:
            raise IndexError(f"Could not read frame {entry}")
        return entry / self.fps, cv2.cvtColor(frame, cv2.COLOR_BGR2RGB)

    def __del__(self):
        if hasattr(self, "cap"):
            self.cap.release()


def load_dataset(path, dataset_type: Optional[str] = None, calibration=None) -> Dataset:
    """dataset_type: "folder" | "tum" | "euroc" | "video", or None to detect it: a video suffix, then rgb.txt or rgb/
    (TUM), then mav0/ or cam0/ (EuRoC), else a folder of images.  calibration: a CameraModel, a calibration file or a
    mapping (camera.load_calibration) used in place of the file beside the frames, which is then not opened."""
    path = Path(os.fspath(path))
    if dataset_type is None:
        if path.suffix.lower() in VIDEO_EXTENSIONS:
            dataset_type = "video"
        elif (path / "rgb.txt").exists() or (path / "rgb").exists():
            dataset_type = "tum"
        elif (path / "mav0").exists() or (path / "cam0").exists():
            dataset_type = "euroc"
        else:
            dataset_type = "folder"
    readers = {"folder": FolderDataset, "tum": TUMDataset, "euroc": EuRoCDataset, "video": VideoDataset}
    if dataset_type not in readers:
        raise ValueError(f"Unknown dataset type: {dataset_type}")
    return readers[dataset_type](path, calibration=calibration)
