"""Minimal SLAM driver over the hot-path operators: the control flow of
/root/reference/src/mlx_mast3r_slam/slam.py (:124-153 main loop, :159-214 INIT / TRACKING,
:216-290 RELOC, :292-318 backend).  It exists to show the operator API dropping in under the loop and to
test it end to end; visualisation stays out of scope.  run_dataset reads a dataset (mast3r_slam/dataloader.py) and
resizes its frames on the device (mast3r_slam/preprocess.py).  The map and trajectory writers
(:320-415) are save_pointcloud / save_trajectory / reconstruction over mast3r_slam/export.py.

Relocalization is opt-in: SLAM(model, retrieval=db_or_True) keeps a keyframe retrieval database
(mast3r_slam/retrieval.py) fed on INIT and on every new keyframe, and a frame that cannot be tracked is matched
against the retrieved keyframes (:216-290).  With retrieval=None (the default) a frame that cannot be tracked is
re-initialised as a new keyframe at the last keyframe's pose (the reference's "no similar keyframes" branch,
:280-286).  loop_closure=True (an extension, also opt-in) adds each new keyframe's retrieved candidates outside the
three-keyframe window to its backend edges; the reference computes these candidates (:211) and discards them.
"""
from __future__ import annotations

import math
from collections import deque
from typing import Callable, Iterable, Optional

import torch

from . import export, fusion, intrinsics, render
from .config import get_config
from .consistency import consistent_keyframes
from .dataloader import Dataset, load_dataset
from .frame import Keyframes, create_frame
from .global_opt import FactorGraph
from .mast3r_utils import mast3r_inference_mono, mast3r_match_asymmetric, mast3r_match_symmetric
from .preprocess import adjust_intrinsics, resize_geometry
from .retrieval import RetrievalDatabase, load_retriever
from .tracker import FrameTracker, sim3_act

INIT, TRACKING, RELOC = "INIT", "TRACKING", "RELOC"


class SLAM:
    def __init__(self, model, K: Optional[torch.Tensor] = None, retrieval=None, loop_closure: bool = False) -> None:
        self.model = model
        self.config = get_config()
        self.keyframes = Keyframes()
        if K is not None:
            self.keyframes.set_intrinsics(K)
        self._K_raw = K                               # as given: run_dataset adjusts it to the preprocessed frames
        self.tracker = FrameTracker(model, self.keyframes)
        self.factor_graph = FactorGraph(model, self.keyframes, K if self.config.get("use_calib") else None)
        self.mode = INIT
        self._queue: deque[int] = deque()
        self.timestamps: list = []
        self.poses: list[torch.Tensor] = []
        # retrieval: a RetrievalDatabase, True (one built by load_retriever) or None (no relocalization database)
        if retrieval is True:
            retrieval = load_retriever(model)
        if retrieval is not None and not isinstance(retrieval, RetrievalDatabase):
            raise TypeError(f"retrieval must be a RetrievalDatabase, True or None, got {type(retrieval).__name__}")
        self.retrieval_db: Optional[RetrievalDatabase] = retrieval
        if loop_closure and retrieval is None:
            raise ValueError("loop_closure=True needs a retrieval database (retrieval=True or a RetrievalDatabase)")
        self.loop_closure = bool(loop_closure)
        self.retrieval_candidates: dict[int, list[int]] = {}     # keyframe index -> keyframes retrieved when it was added

    # ------------------------------------------------------------------ slam.py:124-153
    def run(self, frames: Iterable, callback: Optional[Callable] = None) -> dict:
        """frames: iterable of (timestamp, img) with img [3,H,W] float in [0,1] or uint8 [H,W,3]."""
        for i, (timestamp, img) in enumerate(frames):
            frame = create_frame(i, img if isinstance(img, torch.Tensor) else torch.as_tensor(img))
            frame.img = frame.img.to(self.model.device)
            frame.K = self.keyframes.get_intrinsics()
            if self.mode == INIT:
                self._process_init(frame)
            elif self.mode == TRACKING:
                self._process_tracking(frame)
            else:
                self._process_reloc(frame)
            self.timestamps.append(timestamp)
            self.poses.append(frame.T_WC)
            if callback:
                callback(frame, self.keyframes)
            self._run_backend()
        return self.results()

    def run_dataset(self, dataset_or_path, dataset_type: Optional[str] = None, callback: Optional[Callable] = None) -> dict:
        """slam.py:93-96 of the reference: load a dataset (a path, or a Dataset), resize and crop its frames on the
        device to config["dataset"]["img_size"], move the intrinsics the driver was given to the preprocessed image,
        and run.  A dataset with a calibration is undistorted on the device first and brings its own intrinsics
        (Dataset.intrinsics): giving the driver a K as well is an error."""
        ds = dataset_or_path if isinstance(dataset_or_path, Dataset) else load_dataset(dataset_or_path, dataset_type)
        undistort = ds.calibration is not None and bool(self.config["dataset"].get("undistort", True))
        if undistort and self._K_raw is not None:
            raise ValueError("run_dataset: two sources of intrinsics: SLAM(model, K=...) was given a K and the dataset "
                             f"has a calibration ({ds.calibration!r}); drop one of them")
        if undistort:
            K = torch.from_numpy(ds.intrinsics(self.config["dataset"]["img_size"]))
            self.keyframes.set_intrinsics(K)
            if self.config.get("use_calib"):
                self.factor_graph.K = K
        elif self._K_raw is not None and len(ds):
            h, w = ds[0][1].shape[:2]
            K = adjust_intrinsics(self._K_raw, resize_geometry(h, w, self.config["dataset"]["img_size"])[3])
            self.keyframes.set_intrinsics(K)
            if self.factor_graph.K is not None:
                self.factor_graph.K = K
        return self.run(ds.frames(self.model.device, size=self.config["dataset"]["img_size"]), callback)

    def _mono(self, frame) -> None:
        X, C, feat, pos = mast3r_inference_mono(self.model, frame)
        frame.N, frame.N_updates = 0, 0
        frame.update_pointmap(X, C)                     # the frame owns its fusion buffers
        frame.feat, frame.pos = feat, pos

    def _add_keyframe(self, frame) -> None:
        self.keyframes.append(frame)
        self._queue.append(len(self.keyframes) - 1)

    def _retrieval_update(self, frame, add_after_query: bool) -> list[int]:
        r = self.config.get("retrieval", {})            # absent from DEFAULT_CONFIG: the reference's values (config.py)
        return self.retrieval_db.update(frame, add_after_query=add_after_query, k=r.get("k", 3),
                                        min_thresh=r.get("min_thresh", 0.005))

    def _register_keyframe(self, frame) -> None:
        """Database row i is keyframe i: insert the keyframe just appended and keep what it retrieved."""
        self.retrieval_candidates[len(self.keyframes) - 1] = self._retrieval_update(frame, add_after_query=True)
        assert len(self.retrieval_db) == len(self.keyframes)

    def _process_init(self, frame) -> None:             # :159-182
        self._mono(frame)
        self._add_keyframe(frame)
        if self.retrieval_db is not None:
            self._register_keyframe(frame)
        self.mode = TRACKING

    def _process_tracking(self, frame) -> None:         # :184-214
        new_kf, _, try_reloc = self.tracker.track(frame, mast3r_match_fn=mast3r_match_asymmetric)
        if try_reloc:
            self.mode = RELOC
            self._process_reloc(frame)
            return
        if new_kf:
            self._mono(frame)
            self._add_keyframe(frame)
            if self.retrieval_db is not None:
                self._register_keyframe(frame)

    def _process_reloc(self, frame) -> None:            # :216-290
        if self.retrieval_db is not None:
            self._process_reloc_retrieval(frame)
            return
        self._mono(frame)
        last = self.keyframes.last_keyframe()
        if last is not None:
            frame.T_WC = last.T_WC.clone()
        self._add_keyframe(frame)
        self.mode = TRACKING
        self.tracker.reset_idx_f2k()

    def _process_reloc_retrieval(self, frame) -> None:  # :216-290 with the retrieval database
        self._mono(frame)
        candidates = self._retrieval_update(frame, add_after_query=False)
        if candidates:
            self.keyframes.append(frame)
            kf_idx = len(self.keyframes) - 1
            min_match_frac = self.config["reloc"]["min_match_frac"]
            for cand in candidates:
                if self.factor_graph.add_factors([kf_idx], [cand], min_match_frac, mast3r_match_fn=mast3r_match_symmetric):
                    frame.T_WC = self.keyframes[cand].T_WC.clone()
                    self._register_keyframe(frame)
                    if self.config.get("use_calib"):
                        self.factor_graph.solve_GN_calib()
                    else:
                        self.factor_graph.solve_GN_rays()
                    break
            else:
                self.keyframes.pop_last()
        else:
            self._add_keyframe(frame)
            self._register_keyframe(frame)
        assert len(self.retrieval_db) == len(self.keyframes)
        self.mode = TRACKING
        self.tracker.reset_idx_f2k()

    def _run_backend(self) -> None:                     # :292-318
        while self._queue:
            idx = self._queue.popleft()
            if idx > 0:
                ii = list(range(max(0, idx - 3), idx))
                if self.loop_closure and self.retrieval_db is not None:     # retrieved keyframes outside the window
                    ii = ii + [c for c in self.retrieval_candidates.get(idx, []) if c < ii[0]]
                self.factor_graph.add_factors(ii, [idx] * len(ii),
                                              min_match_frac=self.config["local_opt"].get("min_match_frac", 0.1),
                                              mast3r_match_fn=mast3r_match_symmetric)
            if self.config.get("use_calib"):
                self.factor_graph.solve_GN_calib()
            else:
                self.factor_graph.solve_GN_rays()

    def results(self) -> dict:                          # :320-352 (tensors instead of numpy)
        pts = [sim3_act(kf.T_WC, kf.X_canon) for kf in self.keyframes._frames if kf.X_canon is not None]
        return {
            "timestamps": list(self.timestamps),
            "poses": torch.cat(self.poses) if self.poses else torch.empty((0, 8)),
            "points": torch.cat(pts) if pts else torch.empty((0, 3)),
            "keyframe_indices": [kf.frame_id for kf in self.keyframes._frames],
        }

    # ------------------------------------------------------------------ slam.py:320-415
    def _consistent(self, consistency, c_conf_threshold):
        """(keyframes, threshold) for the map writers under `consistency` (True: consistency.multiview_support's defaults;
        a dict: its keyword arguments).  The pinhole is the keyframes' intrinsics (the K the driver was given, moved to the
        preprocessed frames) when there are any, else "estimate".  The
        filter's own confidence test is c_conf_threshold unless the dict sets one; a threshold of None is passed on as
        -inf, so that "every point" still means every KEPT point (a rejected point's confidence is -inf)."""
        kw = {} if consistency is True else dict(consistency)
        kw.setdefault("c_conf_threshold", c_conf_threshold)
        K = self.keyframes.get_intrinsics()
        frames = consistent_keyframes(self.keyframes, "estimate" if K is None else K, **kw)
        return frames, (-math.inf if c_conf_threshold is None else c_conf_threshold)

    def reconstruction(self, c_conf_threshold: Optional[float] = 1.5, voxel_size: Optional[float] = None,
                       return_index: bool = False, consistency=None):
        """export.collect_map over the keyframes: (points [M,3] float32, colours [M,3] uint8[, index [M] int64]).
        consistency: None - no cross-check between keyframes; True or a dict of consistency.multiview_support's keyword
        arguments - only points that pass the multi-view consistency filter (see _consistent)."""
        if consistency is None or consistency is False:
            return export.collect_map(self.keyframes, c_conf_threshold=c_conf_threshold, voxel_size=voxel_size,
                                      return_index=return_index)
        frames, thr = self._consistent(consistency, c_conf_threshold)
        return export.collect_map(frames, c_conf_threshold=thr, voxel_size=voxel_size, return_index=return_index)

    def save_pointcloud(self, path, c_conf_threshold: Optional[float] = 1.5, voxel_size: Optional[float] = None,
                        binary: bool = True, consistency=None) -> int:
        """:383-415 as a filtered (and optionally voxel-thinned) PLY; returns the number of vertices written.
        consistency as for reconstruction."""
        points, colors = self.reconstruction(c_conf_threshold, voxel_size, consistency=consistency)
        return export.save_ply(path, points, colors, binary=binary)

    def mesh(self, c_conf_threshold: Optional[float] = 1.5, stride: int = 1, edge_ratio: Optional[float] = None,
             return_index: bool = False, consistency=None):
        """export.collect_mesh over the keyframes: (vertices [V,3] float32, colours [V,3] uint8, faces [F,3] int32
        [, index [V] int64]).  Opt-in: nothing in the loop uses it.  consistency as for reconstruction."""
        if consistency is None or consistency is False:
            return export.collect_mesh(self.keyframes, c_conf_threshold=c_conf_threshold, stride=stride, edge_ratio=edge_ratio,
                                       return_index=return_index)
        frames, thr = self._consistent(consistency, c_conf_threshold)
        return export.collect_mesh(frames, c_conf_threshold=thr, stride=stride, edge_ratio=edge_ratio, return_index=return_index)

    def save_mesh(self, path, c_conf_threshold: Optional[float] = 1.5, stride: int = 1,
                  edge_ratio: Optional[float] = None, binary: bool = True):
        """The keyframes' triangle mesh as a PLY with a face element; returns (vertices, faces) written.  For a mesh of
        the consistency-filtered map write export.save_ply_mesh(path, *self.mesh(..., consistency=True))."""
        vertices, colors, faces = self.mesh(c_conf_threshold, stride, edge_ratio)
        return export.save_ply_mesh(path, vertices, colors, faces, binary=binary)

    def fused_mesh(self, voxel_size: Optional[float] = None, trunc: Optional[float] = None,
                   c_conf_threshold: Optional[float] = 1.5, min_weight: int = 1, consistency=None, bounds=None):
        """One connected surface of the whole map: fusion.fuse_tsdf over the keyframes and their current poses, then
        fusion.extract_surface: (vertices [V,3] float32, colours [V,3] uint8, faces [F,3] int32).  Opt-in: nothing in the
        loop uses it.  The pinhole is the keyframes' intrinsics when there are any, else "estimate".  bounds None: the box of
        the exported points (fusion.map_bounds); voxel_size None: the longest side of the bounds over 256; trunc None:
        4 * voxel_size.  These defaults and min_weight = 1 are this project's choice, untuned on real data.  consistency
        as for reconstruction.  No keyframes: an empty mesh."""
        if consistency is None or consistency is False:
            frames, thr = self.keyframes, c_conf_threshold
        else:
            frames, thr = self._consistent(consistency, c_conf_threshold)
        if not export._with_pointmap(frames):
            return export._empty_mesh("cuda" if torch.cuda.is_available() else "cpu", False)
        if bounds is None:
            bounds = fusion.map_bounds(frames, thr)
        if voxel_size is None:
            side = max(float(h) - float(l) for l, h in zip(*bounds))
            if not side > 0.0:
                raise ValueError("the bounds have no extent: pass voxel_size")
            voxel_size = side / 256.0
        K = self.keyframes.get_intrinsics()
        volume = fusion.fuse_tsdf(frames, "estimate" if K is None else K, voxel_size, bounds=bounds, trunc=trunc,
                                  c_conf_threshold=thr)
        return fusion.extract_surface(volume, min_weight=min_weight)

    def save_fused_mesh(self, path, voxel_size: Optional[float] = None, trunc: Optional[float] = None,
                        c_conf_threshold: Optional[float] = 1.5, min_weight: int = 1, consistency=None, bounds=None,
                        binary: bool = True):
        """fused_mesh as a PLY with a face element, written by export.save_ply_mesh; returns (vertices, faces) written."""
        vertices, colors, faces = self.fused_mesh(voxel_size, trunc, c_conf_threshold, min_weight, consistency, bounds)
        return export.save_ply_mesh(path, vertices, colors, faces, binary=binary)

    def save_trajectory(self, path, format: str = "tum", keyframes_only: bool = False) -> int:
        """:354-381.  Default: every processed frame at the pose it was given (results()["poses"]).  keyframes_only:
        the keyframes' current, backend-optimised poses at their own timestamps."""
        if keyframes_only:
            kfs = self.keyframes._frames
            ts = [self.timestamps[kf.frame_id] for kf in kfs]
            poses = self.keyframes.get_poses() if kfs else torch.empty((0, 8))
        else:
            ts = self.timestamps
            poses = torch.cat(self.poses) if self.poses else torch.empty((0, 8))
        return export.save_trajectory(path, ts, poses, format=format)

    def estimate_intrinsics(self, **kw) -> intrinsics.IntrinsicsEstimate:
        """intrinsics.estimate_intrinsics over the keyframes: one pinhole for the map from the pointmaps themselves.
        Opt-in: nothing in the loop uses it."""
        return intrinsics.estimate_intrinsics(self.keyframes, **kw)

    # ------------------------------------------------------------------ headless views (no counterpart: the reference
    # hands its callback to a desktop GUI)
    def render_view(self, T_WC: Optional[torch.Tensor] = None, K=None, size=None, surface: str = "points", mesh_kw=None,
                    **kw):
        """render.render_map over the keyframes: (rgb uint8 [H,W,3], depth float32 [H,W][, index]).  Defaults: the pose
        the last processed frame was given, the keyframes' own image size, and the keyframes' intrinsics moved to
        `size` (render.default_intrinsics without calibration).  K = "estimate": the pinhole of estimate_intrinsics()
        moved to `size` (one host read of the per-keyframe focals).

        surface "mesh" draws self.mesh(**mesh_kw) and "fused" self.fused_mesh(**mesh_kw) with render.render_mesh (solid
        surfaces; `kw` are then render_mesh's, and index is the face index; shading="headlight" lights the surface from
        the eye, normals.py); "points" is render_map as above."""
        if surface not in ("points", "mesh", "fused"):
            raise ValueError(f"render_view: surface must be 'points', 'mesh' or 'fused', got {surface!r}")
        if mesh_kw and surface == "points":
            raise ValueError("render_view: mesh_kw is for surface='mesh' or 'fused'")
        if surface == "points" and any(kw.get(k) is not None for k in ("shading", "normals", "shade_kw")):
            raise ValueError("render_view: shading is for surface='mesh' or 'fused': points carry no normals")
        frames = [kf for kf in self.keyframes._frames if kf.X_canon is not None]
        if T_WC is None:
            if not self.poses:
                raise ValueError("render_view: no frame has been processed yet; pass T_WC")
            T_WC = self.poses[-1]
        own = render._frame_size(frames[0].img) if frames else None
        if size is None:
            if own is None:
                raise ValueError("render_view: the map is empty; pass size")
            size = own
        if K is None and own is not None and self.keyframes.get_intrinsics() is not None:
            K = render.scaled_intrinsics(self.keyframes.get_intrinsics(), own, size)
        if isinstance(K, str):
            if K != "estimate":
                raise ValueError(f"render_view: K must be intrinsics, None or 'estimate', got {K!r}")
            est = self.estimate_intrinsics()
            K = render.scaled_intrinsics(est.K, est.size, size)
        if surface == "points":
            return render.render_map(self.keyframes, T_WC, K, size, **kw)
        mesh = (self.mesh if surface == "mesh" else self.fused_mesh)(**(mesh_kw or {}))
        return render.render_mesh(*mesh[:3], T_WC, K, size, **kw)

    def save_view(self, path, T_WC: Optional[torch.Tensor] = None, K=None, size=None, surface: str = "points",
                  mesh_kw=None, **kw) -> None:
        """render_view written as a PNG."""
        render.save_image(path, self.render_view(T_WC, K, size, surface=surface, mesh_kw=mesh_kw, **kw)[0])
