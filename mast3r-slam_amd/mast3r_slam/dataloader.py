"""Dataset readers (the behaviour of the reference's dataloader.py:37-268: folder, TUM, EuRoC, video, load_dataset) and
the step from a camera-sized frame to a network-sized one on the device (Dataset.frames over
preprocess.resize_img_device).  Decoding stays on the host (PIL / cv2); resizing and cropping do not.

A dataset is a sequence of (timestamp, uint8 [H,W,3] numpy RGB).  `dataset.subsample` / `dataset.reverse` of the
config are read when a reader is built, as in the reference.
"""
from __future__ import annotations

import os
from pathlib import Path
from typing import Iterator, Optional, Sequence

import numpy as np
import torch

from .config import get_config
from .preprocess import resize_img_device

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
    def frames(self, device, size: Optional[int] = None, square_ok: bool = False, batch: int = 1):
        """Generator of (timestamp, uint8 [H',W',3] on `device`): each raw frame is uploaded as it was decoded and
        resized + cropped there (resize_img_device).  `batch` frames share one upload and one launch while their
        source shapes agree.  size None: config["dataset"]["img_size"].  This is what SLAM.run takes."""
        if size is None:
            size = get_config()["dataset"]["img_size"]
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"frames: must target the ROCm device (got {device}); no CPU path exists")
        batch = max(int(batch), 1)
        pending: list = []

        def flush():
            raw = np.stack([f for _, f in pending]) if len(pending) > 1 else pending[0][1][None]
            out = resize_img_device(torch.from_numpy(np.ascontiguousarray(raw)).to(device), size, square_ok)
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

    def __init__(self, frames: Sequence, timestamps: Optional[Sequence[float]] = None) -> None:
        super().__init__()
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

    def __init__(self, path, extensions: Sequence[str] = IMAGE_EXTENSIONS) -> None:
        super().__init__()
        self.path = Path(path)
        self.extensions = tuple(extensions)
        self._entries = sorted(f for f in self.path.iterdir() if f.suffix.lower() in self.extensions)
        self._finish(f"No images found in {path} with extensions {self.extensions}")
        self.images = self._entries

    def _load(self, entry, idx):
        return float(idx), _read_rgb(entry)


class TUMDataset(Dataset):
    """TUM RGB-D layout: rgb.txt (or associated.txt) lines "timestamp path", `#` lines skipped; without either file
    the rgb/*.png files, whose names are the timestamps."""

    def __init__(self, path) -> None:
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

    def _load(self, entry, idx):
        return entry[0], _read_rgb(entry[1])


class EuRoCDataset(Dataset):
    """EuRoC MAV layout: mav0/cam0/data/*.png (or cam0/data), file names are nanosecond timestamps."""

    def __init__(self, path) -> None:
        super().__init__()
        self.path = Path(path)
        cam = self.path / "mav0" / "cam0" / "data"
        if not cam.exists():
            cam = self.path / "cam0" / "data"
        if not cam.exists():
            raise ValueError(f"Camera directory not found in EuRoC dataset at {path}")
        self._entries = [(float(p.stem) / 1e9, p) for p in sorted(cam.glob("*.png"))]
        self._finish(f"No frames found in EuRoC dataset at {path}")

    def _load(self, entry, idx):
        return entry[0], _read_rgb(entry[1])


class VideoDataset(Dataset):
    """A video file decoded by OpenCV; timestamp = frame number / fps."""

    def __init__(self, path) -> None:
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


def load_dataset(path, dataset_type: Optional[str] = None) -> Dataset:
    """dataset_type: "folder" | "tum" | "euroc" | "video", or None to detect it: a video suffix, then rgb.txt or rgb/
    (TUM), then mav0/ or cam0/ (EuRoC), else a folder of images."""
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
    return readers[dataset_type](path)
