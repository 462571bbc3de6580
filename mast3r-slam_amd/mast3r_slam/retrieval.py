"""Keyframe retrieval database on the MI355X: RetrievalDatabase and load_retriever of
/root/reference/src/mlx_mast3r_slam/mast3r_utils.py (:83-114, :640-795), same names, parameters and defaults.

Only the reference's "simple retrieval" exists here (its fallback when the pretrained retrieval head cannot be
loaded, :669-674): the head's weights (RetrievalModel.forward_features / forward_global) are not available, so
`use_simple_retrieval` is always True and `prep_features` raises NotImplementedError.

    signature  = mean over tokens of the encoder features, / sqrt(sum(x^2) + 1e-8)       (:696-715)
    similarity = dot product with every stored signature
    result     = top-k by reversed stable argsort (equal scores: the larger index first), update() keeps sim > min_thresh

Both steps are HIP kernels (csrc/retrieval.hip): the signature is written by the kernel straight into a row of one
device-resident [capacity, C] fp32 buffer that doubles when full (existing rows are copied device to device and keep
their bits), and a query is two launches plus ONE device-to-host copy of (count, idx, score).  Deliberate difference:
the reference takes the mean in the feature dtype (mx.mean of fp16 tokens); here the token sum is fp32 with a fixed
order, so the float64 oracle of the formula above is the yardstick and a signature's bits do not depend on how many
frames are batched with it.  CPU tensors raise RuntimeError: there is no CPU path.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import _ffi

__all__ = ["RetrievalDatabase", "load_retriever"]

_DT = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 3}      # M3_RETRIEVAL_BF16 / _F16 / _F32
MAX_K = 64


def _clamp_k(k: int, rows: int) -> int:
    """k above the kernel's limit is only accepted where it cannot change the result (at most `rows` matches)."""
    k = int(k)
    return min(k, MAX_K) if rows <= MAX_K else k


def load_retriever(model, backbone_dim: Optional[int] = None) -> "RetrievalDatabase":
    """mast3r_utils.py:83-114: a RetrievalDatabase whose dimension is model.embed_dim unless given."""
    if backbone_dim is None:
        backbone_dim = getattr(model, "embed_dim", 1024)
    return RetrievalDatabase(model, backbone_dim=backbone_dim)


class RetrievalDatabase:
    """mast3r_utils.py:640-795 (simple retrieval).  Row i of `signatures` belongs to kf_ids[i]."""

    _INITIAL_CAPACITY = 64

    def __init__(self, model, backbone_dim: int = 1024):
        self.model = model
        self.backbone_dim = int(backbone_dim)
        if self.backbone_dim < 8 or self.backbone_dim % 8:
            raise ValueError(f"backbone_dim must be a positive multiple of 8, got {backbone_dim}")
        self.retrieval = None                       # the pretrained head: not available (see prep_features)
        self.use_simple_retrieval = True
        self.kf_ids: list[int] = []
        self.kf_counter = 0
        self._buf: Optional[torch.Tensor] = None    # [capacity, C] fp32 on the device, allocated on first use
        self._n = 0
        self._ws: Optional[torch.Tensor] = None     # kernel workspace (uint8), grown on demand

    # ------------------------------------------------------------------ storage
    def __len__(self) -> int:
        return self._n

    @property
    def capacity(self) -> int:
        return 0 if self._buf is None else self._buf.shape[0]

    @property
    def signatures(self) -> torch.Tensor:
        """[len, C] view of the device buffer."""
        if self._buf is None:
            return torch.empty((0, self.backbone_dim), dtype=torch.float32)
        return self._buf[:self._n]

    def _device(self, t: torch.Tensor) -> torch.device:
        if not t.is_cuda:
            raise RuntimeError(f"retrieval: features must live on the ROCm device (got {t.device}); no CPU path exists")
        return t.device

    def _reserve(self, rows: int, device: torch.device) -> torch.Tensor:
        """Make room for `rows` rows (capacity doubles); returns the buffer."""
        if self._buf is None:
            cap = self._INITIAL_CAPACITY
            while cap < rows:
                cap *= 2
            self._buf = torch.empty((cap, self.backbone_dim), dtype=torch.float32, device=device)
        elif rows > self._buf.shape[0]:
            cap = self._buf.shape[0]
            while cap < rows:
                cap *= 2
            new = torch.empty((cap, self.backbone_dim), dtype=torch.float32, device=self._buf.device)
            new[:self._n].copy_(self._buf[:self._n])                 # device to device, bits kept
            self._buf = new
        return self._buf

    def _workspace(self, nbytes: int, device: torch.device) -> torch.Tensor:
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device:
            self._ws = torch.empty((max(int(nbytes), 256),), dtype=torch.uint8, device=device)
        return self._ws

    # ------------------------------------------------------------------ kernels
    def _signatures_into(self, feat: torch.Tensor, out: torch.Tensor) -> None:
        """feat [B,T,C] -> rows out[0..B) (out: [>=B, C] fp32 view with unit column stride)."""
        B, T, C = feat.shape
        nbytes = _ffi.lib().m3_retrieval_signature_ws_bytes(B, T, C)
        ws = self._workspace(nbytes, feat.device)
        _ffi.call("m3_retrieval_signature", _ffi.ptr(feat), _ffi.ptr(out), out.stride(0), _ffi.ptr(ws), ws.numel(),
                  B, T, C, _DT[feat.dtype], _ffi.stream_ptr())

    def _as_tokens(self, features: torch.Tensor) -> torch.Tensor:
        if not isinstance(features, torch.Tensor):
            raise TypeError(f"features: expected a torch.Tensor, got {type(features).__name__}")
        self._device(features)
        if features.dtype not in _DT:
            raise TypeError(f"features: expected float16, bfloat16 or float32, got {features.dtype}")
        if features.shape[-1] != self.backbone_dim:
            raise ValueError(f"features: last dimension {features.shape[-1]} != backbone_dim {self.backbone_dim}")
        if features.dim() == 1:
            return features.reshape(1, 1, -1).contiguous()          # a 1-D input is only normalised (:707-708)
        if features.dim() == 2:
            return features[None].contiguous()
        if features.dim() == 3:
            return features.contiguous()
        raise ValueError(f"features: expected [C], [T,C] or [B,T,C], got {tuple(features.shape)}")

    def _topk(self, qsig: torch.Tensor, n: int, k: int, min_thresh: Optional[float], causal: bool):
        """Queries qsig [Q,C] (a view into the buffer, or a separate tensor) against rows [0, n) (+q with causal).
        Returns per query (rows, scores) as host lists; one device-to-host copy."""
        Q, C = qsig.shape
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k must be in [1, {MAX_K}], got {k}")
        dev = qsig.device
        db = self._buf if self._buf is not None else qsig
        nbytes = _ffi.lib().m3_retrieval_ws_bytes(n, Q, k, int(causal))
        ws = self._workspace(nbytes, dev)
        res = torch.empty((Q * (1 + 2 * k),), dtype=torch.int32, device=dev)     # count [Q] | idx [Q,k] | score [Q,k]
        count, idx = res[:Q], res[Q:Q + Q * k]
        score = res[Q + Q * k:].view(torch.float32)
        _ffi.call("m3_retrieval_topk", _ffi.ptr(qsig), qsig.stride(0), _ffi.ptr(db), db.stride(0), n, Q, C, k,
                  0 if min_thresh is None else 1, float(min_thresh or 0.0), int(causal), _ffi.ptr(count), _ffi.ptr(idx),
                  _ffi.ptr(score), _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr())
        h = res.cpu()
        cnt = h[:Q].tolist()
        hi = h[Q:Q + Q * k].view(Q, k).tolist()
        hs = h[Q + Q * k:].view(torch.float32).view(Q, k).tolist()
        return [(hi[q][:cnt[q]], hs[q][:cnt[q]]) for q in range(Q)]

    # ------------------------------------------------------------------ reference API
    def prep_features(self, features):
        """mast3r_utils.py:679-694 applies the pretrained retrieval head (RetrievalModel.forward_features)."""
        raise NotImplementedError("prep_features needs the pretrained retrieval head (RetrievalModel.forward_features, "
                                  "whitening), whose weights are not available; only simple retrieval is provided")

    def compute_signature(self, features: torch.Tensor) -> torch.Tensor:
        """mast3r_utils.py:696-715: [T,C] -> [C], [B,T,C] -> [B,C], [C] -> [C] (normalised only); fp32 on the device."""
        tok = self._as_tokens(features)
        out = torch.empty((tok.shape[0], self.backbone_dim), dtype=torch.float32, device=tok.device)
        self._signatures_into(tok, out)
        return out if features.dim() == 3 else out[0]

    def update(self, frame, add_after_query: bool = True, k: int = 3, min_thresh: float = 0.0) -> list[int]:
        """mast3r_utils.py:717-768: query the stored signatures (sim > min_thresh, at most k), then insert the frame's
        signature when add_after_query - a frame never retrieves itself.  Returns kf_ids of the matches."""
        return self.update_batch([frame], add_after_query=add_after_query, k=k, min_thresh=min_thresh)[0]

    def update_batch(self, frames: Sequence, add_after_query: bool = True, k: int = 3,
                     min_thresh: float = 0.0) -> list[list[int]]:
        """B frames at once: one signature launch and one query call.  Frame b sees only the rows inserted before it
        (the database's rows and, with add_after_query, frames 0..b-1), so the result equals B sequential update()."""
        from .mast3r_utils import _feat
        frames = list(frames)
        if not frames:
            return []
        feats = [_feat(self.model, f) for f in frames]
        tok = torch.stack([self._as_tokens(f)[0] for f in feats]) if len(feats) > 1 else self._as_tokens(feats[0])
        B = tok.shape[0]
        n = self._n
        buf = self._reserve(n + B, tok.device)
        rows = buf[n:n + B]                                            # signatures land where they will be stored
        self._signatures_into(tok, rows)
        ids = self.kf_ids + (list(range(self.kf_counter, self.kf_counter + B)) if add_after_query else [])
        out: list[list[int]] = [[] for _ in range(B)]
        seen = n + (B - 1 if add_after_query else 0)                  # rows the last query sees
        if k >= 1 and seen > 0:
            for b, (r, _) in enumerate(self._topk(rows, n, _clamp_k(k, seen), float(min_thresh), bool(add_after_query))):
                out[b] = [ids[i] for i in r]                          # rows >= n: frames earlier in this batch
        if add_after_query:
            self._n = n + B
            self.kf_ids = ids
            self.kf_counter += B
        return out

    def query(self, features: torch.Tensor, k: int = 3) -> tuple[list[int], list[float]]:
        """mast3r_utils.py:770-795: (kf_ids, scores) of the k best stored signatures, no threshold."""
        if self._n == 0:
            return [], []
        sig = self.compute_signature(features).reshape(-1, self.backbone_dim)[:1]
        if k < 1:
            return [], []
        r, s = self._topk(sig, self._n, _clamp_k(k, self._n), None, False)[0]
        return [self.kf_ids[i] for i in r], s
