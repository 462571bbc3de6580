"""Two-view MASt3R network on the MI355X (the `model` object of the operator API).

Replaces the reference's external network package: `Mast3rFull.from_pretrained`, `.encode`,
`.reconstruct`, `.embed_dim` (call sites /root/reference/src/mlx_mast3r_slam/mast3r_utils.py:
67-76, 104-109, 278-294, 347-355, 418-421).  The reference tree carries no source or weights
for it (un-vendored submodule thirdparty/mlx-mast3r), so the architecture is the public
MASt3R ViT-L/16 + base decoder + catmlp+dpt head (see oracle/model.py for the layer list) and
weights are either random-initialised (seeded) or loaded from a state dict that uses the public
checkpoint's key names.

Precision (`load_mast3r(..., precision)`, mast3r_utils.py:47-52 accepts "fp16" | "fp32" | "bf16"): the 16-bit
storage type of GEMM operands; accumulation, residual stream, LayerNorm statistics, softmax and all outputs
are fp32 in every mode.
  * "bf16" (BASELINE configs[1]): ViT trunk (encoder + decoders) on v_mfma_f32_16x16x32_bf16; the two heads
    (DPT conv chain, local-feature MLP) on v_mfma_f32_16x16x32_f16 - same MFMA rate.  Measured on the fp32 oracle
    at full depth (scratch study recorded in DESIGN.md section 4): with bf16 everywhere the head's roundings alone move
    the pointmap by 9.7e-4 rel-L2 (trunk: 3.7e-4), with fp16 heads the total is ~4e-4.  `head_precision="bf16"`
    gives the all-bf16 variant.
  * "fp16" (the reference's default): every operand fp16 (3 more mantissa bits, range 65504).
  * "fp32": there is no fp32 MFMA GEMM path worth running (1/16 of the 16-bit rate); the request is served by
    the most precise mode, "fp16" operands with fp32 accumulation - documented cast, not an error.

Device-side design (all kernels are hand-written HIP behind include/m3slam_model.h):
  * activations entering a GEMM are 16-bit (see above), every GEMM accumulates in fp32 on MFMA;
  * the residual stream stays fp32 (GEMM epilogue `C = R + acc + bias`), LayerNorm reads it
    and writes the bf16 GEMM operand - no separate add / cast passes;
  * q, k, v stay interleaved in the projection buffer; RoPE-2D is applied in place to the q|k
    columns and the fused attention kernel reads them through strides;
  * the DPT head runs NHWC so every 3x3 convolution is an implicit GEMM over contiguous
    channel runs; k=s transposed convolutions are GEMMs followed by a pixel un-shuffle.
Batching: all 2P images of P pairs go through the encoder as one [2P*T, 1024] token matrix.
"""
from __future__ import annotations

import math
from typing import Optional

import os

import numpy as np
import torch

from . import ops

FULL_CFG = dict(enc_depth=24, enc_dim=1024, enc_heads=16, dec_depth=12, dec_dim=768, dec_heads=12,
                mlp_ratio=4, feat_dim=256, last_dim=128, desc_dim=24, patch=16, rope_base=100.0,
                layer_dims=(96, 192, 384, 768), hooks=(0, 6, 9, 12))
# A tiny configuration with the same structure, for fast parity tests against the CPU oracle.
TINY_CFG = dict(FULL_CFG, enc_depth=2, dec_depth=4, hooks=(0, 2, 3, 4))


def _round_bf16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(torch.float32)


# Gains of the "trained_like" weight family (init_random_weights): chosen on the fp32 CPU oracle at full depth
# (tools/emul_precision.py --family trained_like --stats) so that the statistics a trained ViT-L shows - and a
# trunc-normal(0.02) network does not - are present: see the docstring.
TRAINED_LIKE = dict(ln_log_sigma=0.55, ln_beta=0.1, qk_gain=5.0, fc1_gain=4.0, fc2_gain=0.25,
                    massive_enc=((17, 24.0), (301, -30.0), (777, 36.0)), massive_dec=((5, 40.0), (412, -48.0)))


def init_random_weights(cfg: Optional[dict] = None, seed: int = 0, std: float = 0.02, family: str = "plain") -> dict:
    """Seeded random weights with the public checkpoint's key names (fp32 CPU tensors whose matrix
    entries are bf16-representable).

    family="plain": trunc-normal(std) matrices, N(0, std) biases, LayerNorm gamma = 1 + N(0, std), beta = N(0, std).
    Such a network is close to the identity: attention logits ~ 0 (uniform softmax), no outlier channels, the
    residual stream dominated by the patch embedding.

    family="trained_like": the same draw, then the statistics of a trained ViT that stress 16-bit operands
    (TRAINED_LIKE): LayerNorm gains log-normal over about a decade (exp N(0, 0.55)) with betas N(0, 0.1); the q and k
    projections (self- and cross-attention) scaled so that softmax rows peak (largest logit of a row ~ 30 and more);
    fc1 scaled so that GELU sees |x| > 6 (fc2 scaled back so the residual stream keeps its order of magnitude); a few
    "massive activation" channels, 50-100x the median magnitude of the stream where they enter (three in the encoder
    through the bias of block 1's fc2, two in each decoder through decoder_embed's bias)."""
    if family not in ("plain", "trained_like"):
        raise ValueError(f"family must be 'plain' or 'trained_like', got {family!r}")
    cfg = cfg or FULL_CFG
    g = torch.Generator().manual_seed(seed)
    w: dict[str, torch.Tensor] = {}

    def mat(*shape):
        t = torch.empty(*shape)
        torch.nn.init.trunc_normal_(t, std=std, a=-2 * std, b=2 * std, generator=g)
        return _round_bf16(t)

    def vec(n, base=0.0):
        return base + torch.randn(n, generator=g) * std

    def linear(p, n, k):
        w[p + ".weight"], w[p + ".bias"] = mat(n, k), vec(n)

    def norm(p, n):
        w[p + ".weight"], w[p + ".bias"] = vec(n, 1.0), vec(n)

    def conv(p, co, ci, k, bias=True):
        w[p + ".weight"] = mat(co, ci, k, k)
        if bias:
            w[p + ".bias"] = vec(co)

    E, D, r = cfg["enc_dim"], cfg["dec_dim"], cfg["mlp_ratio"]
    conv("patch_embed.proj", E, 3, 16)
    for i in range(cfg["enc_depth"]):
        p = f"enc_blocks.{i}"
        norm(p + ".norm1", E); linear(p + ".attn.qkv", 3 * E, E); linear(p + ".attn.proj", E, E)
        norm(p + ".norm2", E); linear(p + ".mlp.fc1", r * E, E); linear(p + ".mlp.fc2", E, r * E)
    norm("enc_norm", E)
    linear("decoder_embed", D, E)
    for name in ("dec_blocks", "dec_blocks2"):
        for i in range(cfg["dec_depth"]):
            p = f"{name}.{i}"
            norm(p + ".norm1", D); linear(p + ".attn.qkv", 3 * D, D); linear(p + ".attn.proj", D, D)
            norm(p + ".norm2", D); norm(p + ".norm_y", D)
            for q in ("projq", "projk", "projv", "proj"):
                linear(p + ".cross_attn." + q, D, D)
            norm(p + ".norm3", D); linear(p + ".mlp.fc1", r * D, D); linear(p + ".mlp.fc2", D, r * D)
    norm("dec_norm", D)
    F_, L = cfg["feat_dim"], cfg["last_dim"]
    ld = cfg["layer_dims"]
    for hname in ("downstream_head1", "downstream_head2"):
        p = hname + ".dpt"
        conv(p + ".act_postprocess.0.0", ld[0], E, 1)
        w[p + ".act_postprocess.0.1.weight"], w[p + ".act_postprocess.0.1.bias"] = mat(ld[0], ld[0], 4, 4), vec(ld[0])
        conv(p + ".act_postprocess.1.0", ld[1], D, 1)
        w[p + ".act_postprocess.1.1.weight"], w[p + ".act_postprocess.1.1.bias"] = mat(ld[1], ld[1], 2, 2), vec(ld[1])
        conv(p + ".act_postprocess.2.0", ld[2], D, 1)
        conv(p + ".act_postprocess.3.0", ld[3], D, 1)
        conv(p + ".act_postprocess.3.1", ld[3], ld[3], 3)
        for i in range(4):
            conv(p + f".scratch.layer_rn.{i}", F_, ld[i], 3, bias=False)
        for i in (1, 2, 3, 4):
            q = p + f".scratch.refinenet{i}"
            for u in ("resConfUnit1", "resConfUnit2"):
                conv(q + f".{u}.conv1", F_, F_, 3); conv(q + f".{u}.conv2", F_, F_, 3)
            conv(q + ".out_conv", F_, F_, 1)
        conv(p + ".head.0", F_ // 2, F_, 3)
        conv(p + ".head.2", L, F_ // 2, 3)
        conv(p + ".head.4", 4, L, 1)
        linear(hname + ".head_local_features.fc1", r * (E + D), E + D)
        linear(hname + ".head_local_features.fc2", (cfg["desc_dim"] + 1) * 256, r * (E + D))
    if family == "trained_like":
        _make_trained_like(w, cfg, g)
    return w


def _make_trained_like(w: dict, cfg: dict, g: torch.Generator) -> None:
    """In place: the plain draw -> the "trained_like" family (init_random_weights)."""
    t = TRAINED_LIKE
    E, D = cfg["enc_dim"], cfg["dec_dim"]
    for k in [k for k in w if ".norm" in k or k.startswith(("enc_norm", "dec_norm"))]:
        n = w[k].shape[0]
        if k.endswith(".weight"):
            w[k] = torch.exp(torch.randn(n, generator=g) * t["ln_log_sigma"])
        else:
            w[k] = torch.randn(n, generator=g) * t["ln_beta"]

    def scale_rows(key, rows, gain):
        w[key + ".weight"][rows] = _round_bf16(w[key + ".weight"][rows] * gain)
        w[key + ".bias"][rows] = w[key + ".bias"][rows] * gain

    blocks = [(f"enc_blocks.{i}", E) for i in range(cfg["enc_depth"])]
    blocks += [(f"{n}.{i}", D) for n in ("dec_blocks", "dec_blocks2") for i in range(cfg["dec_depth"])]
    for p, c in blocks:
        scale_rows(p + ".attn.qkv", slice(0, 2 * c), t["qk_gain"])                 # q | k rows; v untouched
        if p.startswith("dec"):
            scale_rows(p + ".cross_attn.projq", slice(None), t["qk_gain"])
            scale_rows(p + ".cross_attn.projk", slice(None), t["qk_gain"])
        scale_rows(p + ".mlp.fc1", slice(None), t["fc1_gain"])
        w[p + ".mlp.fc2.weight"] = _round_bf16(w[p + ".mlp.fc2.weight"] * t["fc2_gain"])
    if cfg["enc_depth"] > 1:
        for ch, val in t["massive_enc"]:
            w["enc_blocks.1.mlp.fc2.bias"][ch % E] = val
    for ch, val in t["massive_dec"]:
        w["decoder_embed.bias"][ch % D] = val


def load_state_dict(path: str) -> dict:
    """A checkpoint with the public MASt3R key names -> {name: fp32 CPU tensor}.

    Accepts a bare state dict or the public checkpoint layout {"model": state_dict, "args": Namespace, ...}
    (torch.load's weights_only=True default refuses the argparse Namespace, so the wrapper layout is read
    with weights_only=False after a weights_only attempt fails - the file is the user's own checkpoint) and
    .safetensors files.  Keys this network does not use (mask_token, the `dec_blocks*.cross_attn` RoPE
    buffers, the training heads) are ignored; a missing key raises KeyError in `_prepare`."""
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        sd = load_file(path, device="cpu")
    else:
        try:
            sd = torch.load(path, map_location="cpu", weights_only=True)
        except Exception:                                  # noqa: BLE001 - pickled Namespace in the public checkpoint
            sd = torch.load(path, map_location="cpu", weights_only=False)
    if isinstance(sd, dict) and "model" in sd and isinstance(sd["model"], dict):
        sd = sd["model"]
    out = {k: v.detach().float() for k, v in sd.items() if isinstance(v, torch.Tensor)}
    if "patch_embed.proj.weight" not in out:
        raise KeyError(f"{path}: not a MASt3R state dict (no 'patch_embed.proj.weight'; keys like {list(out)[:3]})")
    return out


def _pad_to(t: torch.Tensor, dim: int, size: int) -> torch.Tensor:
    if t.shape[dim] == size:
        return t
    shape = list(t.shape)
    shape[dim] = size - t.shape[dim]
    return torch.cat([t, torch.zeros(shape, dtype=t.dtype)], dim=dim)


def _pair2(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """[2, *a.shape] from two same-shape tensors: a strided view when b directly follows a in the same storage (the two
    halves of a 2-group operator's output), a copy otherwise."""
    if (a.shape == b.shape and a.dtype == b.dtype and a.is_contiguous() and b.is_contiguous()
            and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
            and b.data_ptr() == a.data_ptr() + a.numel() * a.element_size()):
        return torch.as_strided(a, (2,) + tuple(a.shape), (a.numel(),) + tuple(a.stride()))
    return torch.stack([a, b])


def _ceil64(n: int) -> int:
    return (n + 63) // 64 * 64


def _lin(W, name: str, w: str = "w", b: str = "b") -> dict:
    """gemm_ex's weight arguments of projection `name` for one or two groups (W: Mast3rFull._W)."""
    (w0, b0), (w1, b1) = W(name, w, b)
    return dict(w=w0, bias=b0, w1=w1, bias1=b1)


class _F32Stream:
    """The residual stream of Mast3rFull._block as an fp32 tensor x, [M,C] or [2,M,C] (two groups): a projection's operand
    is a LayerNorm launch, a residual product accumulates into x in place.  Every method takes the weight lookup W of its
    launch (Mast3rFull._W), which also says whether that launch has one group or two."""

    def __init__(self, dt):
        self.dt = dt                                             # 16-bit type of the operands

    def init(self, W, name, a):
        """The stream becomes projection `name` of a."""
        self.x = ops.gemm_ex(a, epi=ops.EPI_F32, **_lin(W, name))

    def norm(self, W, n, dtype=None):
        """LayerNorm n of the stream in a 16-bit type (the operands' unless given: enc_norm / dec_norm name theirs)."""
        (g0, b0), (g1, b1) = W(n, "g", "b")
        if g1 is None:
            return ops.layernorm(self.x, g0, b0, dtype=dtype or self.dt)
        return ops.layernorm_grouped2(self.x, g0, b0, g1, b1, dtype=dtype or self.dt)

    final_norm = norm

    def norm_pair(self, W, own, cross):
        """(LayerNorm `own` of each group's rows, LayerNorm `cross` of the OTHER group's rows) from one pass over x."""
        return ops.layernorm_dual2(self.x, W(own, "g", "b"), W(cross, "g", "b"), dtype=self.dt)

    def project(self, W, name, a, epi, swap=False, **kw):
        """Projection `name` of a = norm(...) or one of norm_pair(...); `swap`: a holds the other group's rows (it already does)."""
        return ops.gemm_ex(a, epi=epi, **_lin(W, name), **kw)

    def accumulate(self, W, name, a):
        """x += projection `name` of a."""
        ops.gemm_ex(a, epi=ops.EPI_F32_ACCUM, out=self.x, resid=self.x, **_lin(W, name))

    def round(self, dtype):
        return ops.cast_f32(self.x, dtype)


class _HiLoStream:
    """The same stream with the LayerNorm fold (fp16 trunk): x = hi + lo in two fp16 planes (22 bits) that the residual GEMMs
    update in place together with the rows' statistics; hi is the operand of every projection behind a LayerNorm, whose
    epilogue normalises (.fw / .fb / .fcs weights) - no LayerNorm pass, no 16-bit copy of the stream."""

    def __init__(self, rows, cols, groups, device):
        self.hl = ops.ln_hl_buffers(rows, cols, device, groups=groups)
        self.hi, _, self.st = self.hl

    def init(self, W, name, a):
        ops.gemm_ex(a, epi=ops.EPI_F32, hl=self.hl, **_lin(W, name))

    def norm(self, W, n):
        return self.hi

    def norm_pair(self, W, own, cross):
        return self.hi, self.hi

    def project(self, W, name, a, epi, swap=False, **kw):
        """`swap`: group g multiplies the OTHER group's plane, with that plane's statistics (a_swap)."""
        (s0,), (s1,) = W(name, "fcs")
        return ops.gemm_ex(a, epi=epi, fold_in=(self.st, s0, s1), a_swap=swap, **_lin(W, name, "fw", "fb"), **kw)

    def accumulate(self, W, name, a):
        ops.gemm_ex(a, epi=ops.EPI_F32_ACCUM, hl=self.hl, **_lin(W, name))

    def final_norm(self, W, n, dtype):
        p0, p1 = W(n, "g", "b")
        return ops.layernorm_hl(self.hl, *p0, *p1, dtype=dtype)  # enc_norm / dec_norm stay a kernel (it reads the planes)

    def round(self, dtype):
        if dtype == self.hi.dtype:
            return self.hi.clone()                               # the hi plane IS the stream rounded to fp16
        return ops.cast_f32(ops.hl_to_f32(self.hl), dtype)


class Mast3rFull:
    """Drop-in for the reference's `Mast3rFull` model object (mast3r_utils.py:72-76)."""

    embed_dim = 1024
    patch_size = 16

    _PRECISIONS = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float16}

    def __init__(self, weights: Optional[dict] = None, cfg: Optional[dict] = None, device="cuda",
                 resolution: int = 512, precision: str = "bf16", seed: int = 0,
                 head_precision: Optional[str] = None, features: str = "fp32") -> None:
        if features not in ("fp32", "fp16"):
            raise ValueError(f"features must be 'fp32' or 'fp16', got {features!r}")
        self.desc_dtype = torch.float16 if features == "fp16" else torch.float32    # storage of the `desc` output
        if precision not in self._PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(self._PRECISIONS)}, got {precision!r}")
        if head_precision is not None and head_precision not in self._PRECISIONS:
            raise ValueError(f"head_precision must be one of {sorted(self._PRECISIONS)}, got {head_precision!r}")
        if not torch.cuda.is_available():
            raise RuntimeError("Mast3rFull needs a ROCm device; there is no CPU path")
        self.cfg = dict(cfg or FULL_CFG)
        self.embed_dim = int(self.cfg["enc_dim"])                                 # 1024 for every shipped configuration
        self.device = torch.device(device)
        self.resolution = resolution
        self.precision = precision
        self.tdt = self._PRECISIONS[precision]                                    # trunk operand type
        self.hdt = self._PRECISIONS[head_precision] if head_precision else torch.float16   # heads: fp16 unless asked
        # fp16 trunk: q / k stay fp16, v and the softmax probabilities are bf16 (M3_DT_F16_PVBF16) - the fast attention loop
        # needs bf16's exponent range for P, the logits need fp16's mantissa.  M3_ATTN_PV=fp16 keeps
        # everything fp16 (max-tracking loop, ~20 % slower attention).
        self.pv_bf16 = self.tdt == torch.float16 and os.environ.get("M3_ATTN_PV", "bf16") != "fp16"
        # LayerNorm fold (fp16 trunk only; M3_LN_FOLD=0 restores the LayerNorm kernels): the residual GEMMs also write the 16-bit
        # copy of the stream and its row statistics, the projections that follow a LayerNorm multiply that raw copy by
        # gamma-scaled weights and normalise in their epilogue (ops.gemm_ex) - no LayerNorm pass, no LayerNorm launch.  Costs
        # 7-10 % of the fp16 trunk's error budget (tools/experiments/emul_lnfold.py: rounding the raw stream instead of the
        # normalised values; the bf16 trunk cannot afford it and keeps the kernels).
        self.ln_fold = self.tdt == torch.float16 and os.environ.get("M3_LN_FOLD", "1") != "0"
        # ... and only for stream widths whose statistics have a canonical sum tree (m3_ln_slot_count > 0: multiples of 192 or 256
        # with at most four top nodes - 768, 1024; not e.g. 1280 or 1536): other widths keep the LayerNorm kernels
        if self.ln_fold:
            L = ops._ffi.lib()
            self.ln_fold = all(int(L.m3_ln_slot_count(2, int(self.cfg[k]), g)) > 0 for k, g in (("enc_dim", 1), ("dec_dim", 2)))
        self.host_weights = weights if weights is not None else init_random_weights(self.cfg, seed)
        self._prepare(self.host_weights)
        self._rope_cache = {}

    @classmethod
    def from_pretrained(cls, resolution: int = 512, precision: str = "bf16", weights_path: Optional[str] = None,
                        random_init: bool = False, **kw) -> "Mast3rFull":
        """mast3r_utils.py:72-76.  The reference fetches the checkpoint by name; nothing can be fetched here, so
        `weights_path` must name a torch / safetensors state dict with the public MASt3R key names.  Without it the
        call RAISES - a "pretrained" model with random weights would be a silent downgrade - unless the caller asks
        for seeded random weights explicitly with random_init=True (benchmarks and tests do)."""
        if precision not in cls._PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(cls._PRECISIONS)}, got {precision!r}")
        if weights_path is not None:
            return cls(weights=load_state_dict(weights_path), resolution=resolution, precision=precision, **kw)
        if not random_init:
            raise FileNotFoundError(
                "Mast3rFull.from_pretrained: no weights_path given and checkpoints cannot be downloaded here; pass "
                "weights_path=<state dict with the public MASt3R key names> or random_init=True for seeded random weights")
        return cls(weights=None, resolution=resolution, precision=precision, **kw)

    # ------------------------------------------------------------------ weight preparation
    def _prepare(self, w: dict) -> None:
        dev = self.device
        P: dict[str, torch.Tensor] = {}
        wdt = self.tdt                                          # switched to self.hdt for the head weights below

        def lin(p):
            P[p + ".w"] = w[p + ".weight"].to(dev, wdt).contiguous()
            P[p + ".b"] = w[p + ".bias"].to(dev, torch.float32).contiguous()

        def norm(p):
            P[p + ".g"] = w[p + ".weight"].to(dev, torch.float32).contiguous()
            P[p + ".b"] = w[p + ".bias"].to(dev, torch.float32).contiguous()

        def conv3(p, cin_pad=None, bias=True):
            t = w[p + ".weight"].permute(0, 2, 3, 1)                       # [Co,3,3,Ci]
            if cin_pad:
                t = _pad_to(t, 3, cin_pad)
            P[p + ".w"] = t.to(dev, wdt).contiguous()
            P[p + ".b"] = w[p + ".bias"].to(dev, torch.float32).contiguous() if bias else None

        def conv1(p, kpad=None):
            t = w[p + ".weight"][:, :, 0, 0]
            if kpad:
                t = _pad_to(t, 1, kpad)
            P[p + ".w"] = t.to(dev, wdt).contiguous()
            P[p + ".b"] = w[p + ".bias"].to(dev, torch.float32).contiguous()

        def convT(p, s, kpad=None):
            t = w[p + ".weight"]                                            # [Ci,Co,s,s]
            ci, co = t.shape[0], t.shape[1]
            t = t.permute(2, 3, 1, 0).reshape(s * s * co, ci)               # row (dy*s+dx)*Co+co
            if kpad:
                t = _pad_to(t, 1, kpad)
            P[p + ".w"] = t.to(dev, wdt).contiguous()
            P[p + ".b"] = w[p + ".bias"].repeat(s * s).to(dev, torch.float32).contiguous()

        def fold(dst, npre):
            """Consumer of LayerNorm `npre`: weights with gamma folded in (rounded to the operand type), the column sums of
            those ROUNDED weights (what mean * sum_k W[n][k] must cancel exactly), bias + W . beta."""
            if not self.ln_fold:
                return
            wt, bs = w[dst + ".weight"], w[dst + ".bias"]
            gam, bet = w[npre + ".weight"].double(), w[npre + ".bias"].double()
            wf = (wt.double() * gam[None, :]).to(torch.float32).to(wdt)
            P[dst + ".fw"] = wf.to(dev).contiguous()
            P[dst + ".fcs"] = wf.double().sum(1).to(torch.float32).to(dev).contiguous()
            P[dst + ".fb"] = (bs.double() + wt.double() @ bet).to(torch.float32).to(dev).contiguous()

        # the projections that sit behind a LayerNorm, per block kind: (projection, LayerNorm) - what the fold folds
        folded = dict(enc=(("attn.qkv", "norm1"), ("mlp.fc1", "norm2")),
                      dec=(("attn.qkv", "norm1"), ("cross_attn.projq", "norm2"), ("cross_attn.kv", "norm_y"), ("mlp.fc1", "norm3")))
        c = self.cfg
        w = dict(w)                                             # (the concatenated k|v projections are added under their own names)
        P["patch.w"] = w["patch_embed.proj.weight"].reshape(c["enc_dim"], -1).to(dev, wdt).contiguous()
        P["patch.b"] = w["patch_embed.proj.bias"].to(dev, torch.float32).contiguous()
        for i in range(c["enc_depth"]):
            p = f"enc_blocks.{i}"
            norm(p + ".norm1"); lin(p + ".attn.qkv"); lin(p + ".attn.proj")
            norm(p + ".norm2"); lin(p + ".mlp.fc1"); lin(p + ".mlp.fc2")
            for proj, npre in folded["enc"]:
                fold(f"{p}.{proj}", f"{p}.{npre}")
        norm("enc_norm"); lin("decoder_embed")
        for name in ("dec_blocks", "dec_blocks2"):
            for i in range(c["dec_depth"]):
                p = f"{name}.{i}"
                for s in ("weight", "bias"):
                    w[f"{p}.cross_attn.kv.{s}"] = torch.cat([w[f"{p}.cross_attn.projk.{s}"], w[f"{p}.cross_attn.projv.{s}"]], 0)
                norm(p + ".norm1"); lin(p + ".attn.qkv"); lin(p + ".attn.proj")
                norm(p + ".norm2"); norm(p + ".norm_y"); lin(p + ".cross_attn.projq"); lin(p + ".cross_attn.kv"); lin(p + ".cross_attn.proj")
                norm(p + ".norm3"); lin(p + ".mlp.fc1"); lin(p + ".mlp.fc2")
                for proj, npre in folded["dec"]:
                    fold(f"{p}.{proj}", f"{p}.{npre}")
        norm("dec_norm")
        ld = c["layer_dims"]
        wdt = self.hdt
        for hname in ("downstream_head1", "downstream_head2"):
            p = hname + ".dpt"
            conv1(p + ".act_postprocess.0.0"); convT(p + ".act_postprocess.0.1", 4, _ceil64(ld[0]))
            conv1(p + ".act_postprocess.1.0"); convT(p + ".act_postprocess.1.1", 2, _ceil64(ld[1]))
            conv1(p + ".act_postprocess.2.0"); conv1(p + ".act_postprocess.3.0"); conv3(p + ".act_postprocess.3.1")
            for i in range(4):
                conv3(p + f".scratch.layer_rn.{i}", cin_pad=_ceil64(ld[i]), bias=False)
            for i in (1, 2, 3, 4):
                q = p + f".scratch.refinenet{i}"
                for u in ("resConfUnit1", "resConfUnit2"):
                    conv3(q + f".{u}.conv1"); conv3(q + f".{u}.conv2")
                conv1(q + ".out_conv")
            conv3(p + ".head.0"); conv3(p + ".head.2"); conv1(p + ".head.4")
            lin(hname + ".head_local_features.fc1"); lin(hname + ".head_local_features.fc2")
        self.P = P

    # ------------------------------------------------------------------ helpers
    def _rope(self, gh: int, gw: int):
        """The fused RoPE epilogue's operand for a gh x gw token grid: int32 [T,2] positions (y, x); the kernels compute
        cos/sin of pos * base^(-i/16) themselves (ops.gemm_rope).  rope_base must be ops.ROPE_BASE for the grouped launches."""
        key = (gh, gw)
        if key not in self._rope_cache:
            if float(self.cfg["rope_base"]) != ops.ROPE_BASE:
                raise ValueError(f"rope_base {self.cfg['rope_base']} is not supported by the fused epilogue ({ops.ROPE_BASE})")
            gy, gx = torch.meshgrid(torch.arange(gh), torch.arange(gw), indexing="ij")
            pos = torch.stack([gy.reshape(-1), gx.reshape(-1)], -1).to(torch.int32).to(self.device).contiguous()
            self._rope_cache[key] = ops.rope_bound(pos, max(gh, gw))      # positions < max(gh, gw): the epilogues' LDS cos / sin table
        return self._rope_cache[key]

    def _as_images(self, img) -> torch.Tensor:
        """uint8 [H,W,3] or [B,H,W,3], numpy or tensor -> device uint8 [B,H,W,3]."""
        if isinstance(img, np.ndarray):
            img = torch.from_numpy(np.ascontiguousarray(img))
        if img.dtype != torch.uint8:
            raise TypeError("images must be uint8 [H,W,3] (frame_to_numpy, mast3r_utils.py:210-226)")
        if img.dim() == 3:
            img = img[None]
        if img.shape[-1] != 3 or img.shape[1] % 16 or img.shape[2] % 16:
            raise ValueError(f"images must be [B,H,W,3] with H,W multiples of 16, got {tuple(img.shape)}")
        return img.to(self.device).contiguous()

    def _attn_qkv(self, qkv, nb, t, heads):
        """Self-attention of nb images of t tokens on a packed q|k|v projection [..., 3c] (q|k rotated, q pre-scaled by
        ops.QK_PRESCALE; c = heads * 64): the kernel reads the three column blocks through strides.  -> [..., c]."""
        c = heads * 64
        out = torch.empty(qkv.shape[:-1] + (c,), dtype=qkv.dtype, device=qkv.device)
        f = qkv.view(-1, 3 * c)
        ops.attention(f, f[:, c:], f[:, 2 * c:], out, nbatch=nb, heads=heads, tq=t, tk=t, q_row_stride=3 * c, kv_row_stride=3 * c,
                      o_row_stride=c, q_batch_stride=t * 3 * c, kv_batch_stride=t * 3 * c, o_batch_stride=t * c, prescaled=True,
                      pv_bf16=self.pv_bf16)
        return out

    def _attn_q_kv(self, q, kv, nb, t, heads):
        """Cross-attention of nb images of t tokens: q [..., c] (rotated, pre-scaled) on a packed k|v projection [..., 2c]
        (k rotated) of the same row order.  -> [..., c]."""
        c = heads * 64
        out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        f = kv.view(-1, 2 * c)
        ops.attention(q.view(-1, c), f, f[:, c:], out, nbatch=nb, heads=heads, tq=t, tk=t, q_row_stride=c, kv_row_stride=2 * c,
                      o_row_stride=c, q_batch_stride=t * c, kv_batch_stride=t * 2 * c, o_batch_stride=t * c, prescaled=True,
                      pv_bf16=self.pv_bf16)
        return out

    # ------------------------------------------------------------------ trunk
    def _W(self, p0: str, p1: Optional[str] = None):
        """Weight lookup of a one- or two-group launch: W(name, *fields) -> per group the P[prefix + name.field] of every
        field; the second group's are None for one group (p1 None) - what every operator takes to mean "one group"."""
        P = self.P
        return lambda n, *f: (tuple(P[f"{p0}{n}.{k}"] for k in f), tuple(None if p1 is None else P[f"{p1}{n}.{k}"] for k in f))

    def _stream(self, rows: int, cols: int, groups: int, device):
        """The residual stream of a [rows, cols] (x groups) token matrix.  The fold works on row PAIRS: an odd row count
        (one image with an odd token grid, e.g. 21 x 21) takes the LayerNorm kernels."""
        if self.ln_fold and rows % 2 == 0:
            return _HiLoStream(rows, cols, groups, device)
        return _F32Stream(self.tdt)

    def _block(self, s, W, nb: int, t: int, heads: int, rtok, cross: bool):
        """One transformer block on the residual stream s (either form) of nb images of t tokens: self-attention, with
        `cross` cross-attention on the other group's stream (the decoder), the MLP.  W: the block's weights, one group or two."""
        C, pv, qk = heads * 64, self.pv_bf16, ops.QK_PRESCALE
        if cross:
            # cross-attention memory: norm_y of the OTHER view's previous-layer tokens, then the k|v projection
            # (one pass over the stream also yields norm1 of the same tokens for the self-attention below)
            xn, yn = s.norm_pair(W, "norm1", "norm_y")
            kv = s.project(W, "cross_attn.kv", yn, ops.EPI_BF16_ROPE, swap=True, rope=(rtok, C), pv_bf16=pv)   # [2,M,2C], k rotated
        else:
            xn = s.norm(W, "norm1")
        # [..., 3C], q|k rotated; q additionally carries softmax scale * log2(e) (folded in before the 16-bit rounding)
        qkv = s.project(W, "attn.qkv", xn, ops.EPI_BF16_ROPE, rope=(rtok, 2 * C, C, qk), pv_bf16=pv)
        s.accumulate(W, "attn.proj", self._attn_qkv(qkv, nb, t, heads))
        if cross:
            q = s.project(W, "cross_attn.projq", s.norm(W, "norm2"), ops.EPI_BF16_ROPE, rope=(rtok, C, C, qk))
            s.accumulate(W, "cross_attn.proj", self._attn_q_kv(q, kv, nb, t, heads))
        hdn = s.project(W, "mlp.fc1", s.norm(W, "norm3" if cross else "norm2"), ops.EPI_BF16_GELU)
        s.accumulate(W, "mlp.fc2", hdn)

    def encode_tokens(self, imgs_u8: torch.Tensor, imgs2_u8: Optional[torch.Tensor] = None):
        """uint8 [B,H,W,3] -> (enc_norm tokens, trunk 16-bit type, [B*T,1024], (gh,gw)).  Any H, W that are
        multiples of 16 (resize_img emits e.g. 512x336 -> 672 tokens, 512x288 -> 576).  imgs2_u8 (same shape): a second
        image batch encoded behind the first in the same token matrix ([2B*T,1024]) - both are patchified straight into
        their halves, no concatenated image tensor."""
        c = self.cfg
        b, h, w, _ = imgs_u8.shape
        gh, gw = h // 16, w // 16
        t = gh * gw
        dt = self.tdt
        rtok = self._rope(gh, gw)
        if imgs2_u8 is None:
            patches = ops.patchify16(imgs_u8, dt)
        else:
            patches = torch.empty((2 * b * t, 768), dtype=dt, device=imgs_u8.device)
            ops.patchify16(imgs_u8, dt, out=patches[:b * t])
            ops.patchify16(imgs2_u8, dt, out=patches[b * t:])
            b = 2 * b
        s = self._stream(patches.shape[0], c["enc_dim"], 1, patches.device)
        s.init(self._W(""), "patch", patches)
        for i in range(c["enc_depth"]):
            self._block(s, self._W(f"enc_blocks.{i}."), b, t, c["enc_heads"], rtok, cross=False)
        return s.final_norm(self._W(""), "enc_norm", dt), (gh, gw)

    def encode(self, img):
        """model.encode(img) (mast3r_utils.py:278): uint8 [H,W,3] -> tokens [T,1024] (16-bit tensor of the trunk type);
        a batch [B,H,W,3] gives [B,T,1024]."""
        imgs = self._as_images(img)
        tok, _ = self.encode_tokens(imgs)
        tok = tok.view(imgs.shape[0], -1, self.embed_dim)
        return tok[0] if (not isinstance(img, torch.Tensor) or img.dim() == 3) and imgs.shape[0] == 1 else tok

    # ------------------------------------------------------------------ decoder
    def decode_tokens(self, f1: torch.Tensor, f2: torch.Tensor, npairs: int, grid):
        """f1, f2 [P*T,1024] in the trunk 16-bit type (enc_norm outputs of view 1 / view 2) -> two lists of DPT
        taps ([P*T,C] in the HEAD 16-bit type) at the configured hooks.  The two decoder branches (different
        weights, same shapes) run as 2-group launches: one GEMM / LayerNorm / attention launch serves both views."""
        c = self.cfg
        gh, gw = grid
        t = gh * gw
        rtok = self._rope(gh, gw)
        m = npairs * t
        dt, hdt = self.tdt, self.hdt
        if f1.dtype != dt or f2.dtype != dt:
            raise TypeError(f"encoder features must be {dt} (precision={self.precision!r}), got {f1.dtype}")
        fcat = _pair2(f1, f2)                                     # [2,M,1024]: a view on adjacent halves of the encoder batch
        s = self._stream(m, c["dec_dim"], 2, fcat.device)
        s.init(self._W("", ""), "decoder_embed", fcat)            # both residual streams [2,M,D]
        # tap 0 = the cached encoder features; the heads read them in their own 16-bit type (bf16 -> fp16 is exact
        # for these LayerNorm outputs: fp16 has more mantissa bits and |x| << 65504)
        if hdt == dt:
            taps = [[f1], [f2]]
        else:
            c16 = ops.cast16(fcat.reshape(2 * m, -1), hdt)        # one launch; halves stay adjacent for heads()
            taps = [[c16[:m]], [c16[m:]]]
        for i in range(c["dec_depth"]):
            self._block(s, self._W(f"dec_blocks.{i}.", f"dec_blocks2.{i}."), 2 * npairs, t, c["dec_heads"], rtok, cross=True)
            if i + 1 in c["hooks"]:
                tap = s.final_norm(self._W("", ""), "dec_norm", hdt) if i + 1 == c["dec_depth"] else s.round(hdt)
                taps[0].append(tap[0])
                taps[1].append(tap[1])
        return taps

    # ------------------------------------------------------------------ heads
    def _heads(self, names, taps_per_head, npairs: int, grid):
        """The DPT head + local-feature head of one head (names = (hname,)) or of both as 2-group launches (blockIdx.y =
        head: same shapes, different weights).  Every tensor carries `lead` in front: () for one head, (2,) for two - the
        operators take the second head's weights as w1 / bias1 (None = one group).  taps_per_head: per head, 4 tensors
        [P*T,C] (head 16-bit type).  Returns one dict(pts3d, conf, desc, desc_conf) per head."""
        P, ld = self.P, self.cfg["layer_dims"]
        gh, gw = grid
        m = npairs * gh * gw
        G = len(names)
        lead = (2,) if G == 2 else ()
        dev = taps_per_head[0][0].device
        T = [_pair2(a, b) for a, b in zip(*taps_per_head)] if G == 2 else taps_per_head[0]    # [2,M,C]: a view when the halves are adjacent
        W = lambda s: (P[names[0] + s], P[names[1] + s] if G == 2 else None)
        flat = lambda x: x.reshape((-1,) + tuple(x.shape[-3:]))                      # heads folded into the batch axis (a view)

        def gem(x, s, epi=ops.EPI_BF16, out=None):
            (w0, w1), (b0, b1) = W(s + ".w"), W(s + ".b")
            return ops.gemm_ex(x, w0, b0, epi, out=out, w1=w1, bias1=b1)

        def conv(x, s, epi=ops.EPI_BF16, **kw):
            (w0, w1), (b0, b1) = W(s + ".w"), W(s + ".b")
            return ops.conv3x3_ex(x, w0, b0, epi, w1=w1, bias1=b1, **kw)

        def rcu(x, q):
            c1 = conv(x, q + ".conv1", ops.EPI_BF16_RELU, relu_input=True)           # conv1(relu(x))
            return conv(c1, q + ".conv2", ops.EPI_BF16_ADD, resid=x)

        def fusion(q, x0, x1=None):
            """DPT FeatureFusionBlock WITHOUT its trailing x2 upsample: returns the out_conv output at the block's own
            resolution.  With a skip connection x1, x0 is the previous block's (coarser) output: it is upsampled, cropped
            to x1's size (odd token grids, oracle/model.py dpt_head: path[:, :, :h, :w]) and added to the refined x1 in one
            launch (ops.add_upsample2x) - the upsampled map is never materialised."""
            out = x0
            if x1 is not None:
                y = rcu(x1, q + ".resConfUnit1")
                out = ops.add_upsample2x(flat(x0), flat(y)).view(y.shape)
            # out_conv is 1x1 and the align_corners bilinear weights sum to one, so conv(upsample(x)) ==
            # upsample(conv(x)): run the GEMM on the low-resolution map (4x fewer rows); the consumer upsamples.
            out = rcu(out, q + ".resConfUnit2")
            return gem(out.view(lead + (-1, out.shape[-1])), q + ".out_conv").view(out.shape[:-1] + (-1,))

        def up2(x):
            return ops.upsample2x(flat(x)).view(lead + (npairs, 2 * x.shape[-3], 2 * x.shape[-2], x.shape[-1]))

        d = ".dpt"
        # act_postprocess
        k0, k1 = _ceil64(ld[0]), _ceil64(ld[1])
        t0 = gem(T[0], d + ".act_postprocess.0.0", out=torch.zeros(lead + (m, k0), dtype=self.hdt, device=dev) if k0 != ld[0] else None)
        u0 = gem(t0, d + ".act_postprocess.0.1")
        l0 = ops.unshuffle(u0.view(G * m, -1), G * npairs, gh, gw, 4, ld[0], k0).view(lead + (npairs, 4 * gh, 4 * gw, k0))
        t1 = gem(T[1], d + ".act_postprocess.1.0", out=torch.zeros(lead + (m, k1), dtype=self.hdt, device=dev) if k1 != ld[1] else None)
        u1 = gem(t1, d + ".act_postprocess.1.1")
        l1 = ops.unshuffle(u1.view(G * m, -1), G * npairs, gh, gw, 2, ld[1], k1).view(lead + (npairs, 2 * gh, 2 * gw, k1))
        l2 = gem(T[2], d + ".act_postprocess.2.0").view(lead + (npairs, gh, gw, ld[2]))
        t3 = gem(T[3], d + ".act_postprocess.3.0").view(lead + (npairs, gh, gw, ld[3]))
        l3 = conv(t3, d + ".act_postprocess.3.1", stride=2)
        rn = [conv(l, d + f".scratch.layer_rn.{i}") for i, l in enumerate((l0, l1, l2, l3))]
        path = fusion(d + ".scratch.refinenet4", rn[3])
        path = fusion(d + ".scratch.refinenet3", path, rn[2])
        path = fusion(d + ".scratch.refinenet2", path, rn[1])
        path = fusion(d + ".scratch.refinenet1", path, rn[0])
        if self._direct_head0_ok(path):
            # refinenet1's trailing x2 upsample + head.0 as ONE direct-convolution launch (the 256-channel full-size map is
            # neither written nor gathered nine times)
            (w0, w1), (b0, b1) = W(d + ".head.0.w"), W(d + ".head.0.b")
            h0 = ops.conv3x3_up_direct_ex(path, w0, b0, upsample=True, w1=w1, bias1=b1)
        else:
            h0 = conv(up2(path), d + ".head.0")
        (w2, w21), (w4, w41) = W(d + ".head.2.w"), W(d + ".head.4.w")
        if tuple(w2.shape) == (128, 3, 3, 128) and tuple(w4.shape) == (4, 128):
            # x2 upsample + head.2 conv + ReLU + head.4 1x1 + pointmap post-processing in ONE direct-convolution launch:
            # the full-resolution 128-channel map (537 MB per head at 8 pairs) is never written or read
            (b2, b21), (b4, b41) = W(d + ".head.2.b"), W(d + ".head.4.b")
            pts, conf = ops.dpt_tail_ex(h0, w2, b2, w4, b4, upsample=True, w1=w21, bias1=b21, w41=w41, b41=b41)
        else:                                                                        # another tail geometry: the unfused chain
            h2 = conv(up2(h0), d + ".head.2", ops.EPI_BF16_RELU)
            raw = gem(h2.view(lead + (-1, h2.shape[-1])), d + ".head.4", ops.EPI_F32)
            pts, conf = ops.pts_post(raw.view(h2.shape[:-1] + (4,)))
        # local features
        q = ".head_local_features"
        cat = ops.concat2(T[0].reshape(G * m, -1), T[3].reshape(G * m, -1)).view(lead + (m, -1))
        f = gem(gem(cat, q + ".fc1", ops.EPI_BF16_GELU), q + ".fc2")
        H, Wd = gh * 16, gw * 16
        desc, dconf = ops.desc_post(f.view(G * m, -1), G * npairs, H, Wd, self.desc_dtype)
        out = dict(pts3d=pts, conf=conf, desc=desc.view(lead + (npairs, H, Wd, 24)), desc_conf=dconf.view(lead + (npairs, H, Wd)))
        return (out,) if G == 1 else tuple({k: t[v] for k, t in out.items()} for v in range(2))

    def head(self, hname: str, taps, npairs: int, grid):
        """taps: 4 [P*T,C] tensors in the head 16-bit type -> dict(pts3d [P,H,W,3], conf [P,H,W], desc [P,H,W,24], desc_conf [P,H,W])."""
        return self._heads((hname,), (taps,), npairs, grid)[0]

    def heads(self, taps1, taps2, npairs: int, grid):
        """Both heads (DPT + local features) with every operator as ONE 2-group launch - the form the decoder already uses.
        No side stream: a stream fork here was a second-level fork whenever the caller captured on a forked stream, which
        segfaults inside ROCm 7.2 (tools/incident_r01/nested_capture.py), and the small maps now fill
        twice the CUs.  taps*: 4 tensors [P*T,C] each (head 16-bit type).  Returns (out1, out2) dicts as `head`."""
        return self._heads(("downstream_head1", "downstream_head2"), (taps1, taps2), npairs, grid)

    # ------------------------------------------------------------------ public two-view API
    def reconstruct_batch(self, imgs1: torch.Tensor, imgs2: torch.Tensor):
        """P pairs at once: uint8 [P,H,W,3] x2 -> (out1, out2), dicts with a leading pair axis.
        Both outputs are expressed in view 1's frame (mast3r_utils.py:329-343)."""
        imgs1, imgs2 = self._as_images(imgs1), self._as_images(imgs2)
        if imgs1.shape != imgs2.shape:
            raise ValueError("both views must have the same shape")
        npairs = imgs1.shape[0]
        tok, grid = self.encode_tokens(imgs1, imgs2)
        m = npairs * grid[0] * grid[1]
        return self.decode_heads(tok[:m], tok[m:], npairs, grid)

    def decode_heads(self, f1, f2, npairs, grid):
        """Decoder + both heads from cached encoder tokens (bf16 [P*T,1024] each)."""
        taps = self.decode_tokens(f1.reshape(-1, self.embed_dim), f2.reshape(-1, self.embed_dim), npairs, grid)
        return self.heads(taps[0], taps[1], npairs, grid)

    def _direct_head0_ok(self, path) -> bool:
        """The direct head.0 kernel: 256 (or 128) input channels -> 128, output size (twice the input's) a multiple of 16."""
        w = self.P["downstream_head1.dpt.head.0.w"]
        return (os.environ.get("M3_DIRECT_HEAD0", "1") != "0" and w.shape[0] == 128 and w.shape[3] in (128, 256)
                and (2 * path.shape[-3]) % 16 == 0 and (2 * path.shape[-2]) % 16 == 0)

    def reconstruct(self, img1, img2):
        """model.reconstruct(img1, img2) (mast3r_utils.py:281,355): uint8 [H,W,3] x2 -> two dicts with
        pts3d [H,W,3], conf [H,W,1], desc [H,W,24], desc_conf [H,W] (device tensors)."""
        o1, o2 = self.reconstruct_batch(self._as_images(img1), self._as_images(img2))

        def one(o):
            return dict(pts3d=o["pts3d"][0], conf=o["conf"][0][..., None], desc=o["desc"][0], desc_conf=o["desc_conf"][0])
        return one(o1), one(o2)

    def graphed(self, npairs: int, h: int, w: int) -> "GraphedReconstruct":
        """reconstruct_batch for a fixed (npairs, h, w) captured once into a hipGraph and replayed per call:
        the ~700 kernel launches of a pair cost more host time than GPU time at batch 1."""
        return GraphedReconstruct(self, npairs, h, w)

    def flops_per_pair(self, h: int = 512, w: int = 512) -> float:
        """Algorithmic FLOPs (2*MAC) of one reconstruct() call, from this model's own layer table."""
        c = self.cfg
        t = (h // 16) * (w // 16)
        E, D, r = c["enc_dim"], c["dec_dim"], c["mlp_ratio"]
        enc = c["enc_depth"] * (2 * t * E * 3 * E + 2 * t * E * E + 4 * t * E * r * E + 4 * t * t * E) + 2 * t * 768 * E
        dec = c["dec_depth"] * (2 * t * D * 3 * D + 2 * t * D * D + 4 * t * t * D          # self
                                + 4 * 2 * t * D * D + 4 * t * t * D                          # cross (q,k,v,proj)
                                + 4 * t * D * r * D) + 2 * t * E * D
        feat = 2 * t * (E + D) * r * (E + D) + 2 * t * r * (E + D) * 25 * 256
        F_, ld = c["feat_dim"], c["layer_dims"]
        gh, gw = h // 16, w // 16
        px = [gh * 4 * gw * 4, gh * 2 * gw * 2, gh * gw, ((gh + 1) // 2) * ((gw + 1) // 2)]
        conv = lambda n, ci, co, k: 2.0 * n * ci * co * k * k
        dpt = (conv(t, E, ld[0], 1) + conv(t, ld[0], ld[0] * 16, 1) + conv(t, D, ld[1], 1) + conv(t, ld[1], ld[1] * 4, 1)
               + conv(t, D, ld[2], 1) + conv(t, D, ld[3], 1) + conv(px[3], ld[3], ld[3], 3)
               + sum(conv(px[i], ld[i], F_, 3) for i in range(4))
               + 2 * conv(px[3], F_, F_, 3) + conv(px[3] * 4, F_, F_, 1)
               + sum(4 * conv(px[i], F_, F_, 3) + conv(px[i] * 4, F_, F_, 1) for i in (2, 1, 0))
               + conv(px[0] * 4, F_, F_ // 2, 3) + conv(px[0] * 16, F_ // 2, c["last_dim"], 3) + conv(px[0] * 16, c["last_dim"], 4, 1))
        return 2.0 * (enc + dec + feat + dpt)


class GraphedReconstruct:
    """hipGraph replay of Mast3rFull.reconstruct_batch for one input shape.

    __call__(imgs1, imgs2) copies the uint8 images into the graph's static input buffers, replays, and
    returns the two output dicts.  The outputs are the graph's STATIC buffers: they are overwritten by the
    next call, so consume (or clone) them before calling again.  Stream-ordered on the current stream."""

    def __init__(self, net: Mast3rFull, npairs: int, h: int, w: int) -> None:
        if h % 16 or w % 16 or h <= 0 or w <= 0:
            raise ValueError("H, W must be positive multiples of 16")
        self.net = net
        self.shape = (npairs, h, w, 3)
        self._in1 = torch.zeros(self.shape, dtype=torch.uint8, device=net.device)
        self._in2 = torch.zeros(self.shape, dtype=torch.uint8, device=net.device)
        for _ in range(2):                                   # warm up (lazy attribute setup, allocator pools)
            net.reconstruct_batch(self._in1, self._in2)
        torch.cuda.synchronize(net.device)
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph):
            self._out = net.reconstruct_batch(self._in1, self._in2)

    def __call__(self, imgs1, imgs2):
        imgs1, imgs2 = self.net._as_images(imgs1), self.net._as_images(imgs2)
        if tuple(imgs1.shape) != self.shape or tuple(imgs2.shape) != self.shape:
            raise ValueError(f"captured for images {self.shape}, got {tuple(imgs1.shape)} / {tuple(imgs2.shape)}")
        self._in1.copy_(imgs1)
        self._in2.copy_(imgs2)
        self._graph.replay()
        return self._out
