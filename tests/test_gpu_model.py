"""GPU parity: network operators (through the C ABI) vs plain PyTorch fp32 references of the same
op, and the two-view network end to end vs the torch-CPU fp32 oracle (oracle/model.py).
bf16 storage rounds to 8 significant bits (2^-9 relative), so tolerances are stated per test."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mast3r_slam import mast3r_utils, model as M, ops, synthetic
from mast3r_slam.frame import create_frame
from oracle import model as OM

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float((a.float().cpu() - b.float().cpu()).norm() / b.float().cpu().norm())


DT16 = [torch.bfloat16, torch.float16]
TOL16 = {torch.bfloat16: 3e-3, torch.float16: 4e-4}      # storage rounding 2^-9 / 2^-12 (relative, per element)


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("epi", [ops.EPI_BF16, ops.EPI_BF16_GELU, ops.EPI_F32, ops.EPI_F32_ACCUM, ops.EPI_BF16_RELU,
                                 ops.EPI_BF16_ADD])
@pytest.mark.parametrize("shape", [(256, 256, 128), (300, 132, 64), (2048, 768, 3072), (128, 4, 64)])
def test_gemm_epilogues(dev, epi, shape, dt):
    m, n, k = shape
    g = torch.Generator(device="cpu").manual_seed(m + n + k + epi)
    a = torch.randn(m, k, generator=g).to(dt)
    w = (torch.randn(n, k, generator=g) * 0.05).to(dt)
    b = torch.randn(n, generator=g)
    ref = a.float() @ w.float().T + b
    r = None
    if epi == ops.EPI_BF16_GELU:
        ref = F.gelu(ref)
    if epi == ops.EPI_BF16_RELU:
        ref = torch.relu(ref)
    if epi == ops.EPI_F32_ACCUM:
        r = torch.randn(m, n, generator=g); ref = ref + r
    if epi == ops.EPI_BF16_ADD:
        r = torch.randn(m, n, generator=g).to(dt); ref = ref + r.float()
    out = ops.gemm(a.to(dev), w.to(dev), b.to(dev), epi, resid=None if r is None else r.to(dev))
    f32 = epi in (ops.EPI_F32, ops.EPI_F32_ACCUM)
    assert out.dtype == (torch.float32 if f32 else dt)
    assert _rel(out, ref) < (2e-6 if f32 else TOL16[dt])       # fp32 accumulate; 16-bit output rounding


@pytest.mark.parametrize("epi", [ops.EPI_BF16, ops.EPI_BF16_GELU, ops.EPI_F32_ACCUM, ops.EPI_BF16_ADD])
def test_gemm_192_wide_tiles(dev, epi):
    """16384 x 768 is dispatched to the 256x192 tile variant (256 tiles = one full round of the chip);
    all tile shapes accumulate K in the same order, so a row computed in a small batch (128x128 tiles)
    is bitwise the same."""
    m, n, k = 16384, 768, 128
    g = torch.Generator(device="cpu").manual_seed(11 + epi)
    a = torch.randn(m, k, generator=g).bfloat16()
    w = (torch.randn(n, k, generator=g) * 0.05).bfloat16()
    b = torch.randn(n, generator=g)
    ref = a.float() @ w.float().T + b
    r = None
    if epi == ops.EPI_BF16_GELU:
        ref = F.gelu(ref)
    if epi == ops.EPI_F32_ACCUM:
        r = torch.randn(m, n, generator=g); ref = ref + r
    if epi == ops.EPI_BF16_ADD:
        r = torch.randn(m, n, generator=g).bfloat16(); ref = ref + r.float()
    rd = None if r is None else r.to(dev)
    out = ops.gemm(a.to(dev), w.to(dev), b.to(dev), epi, resid=rd)
    assert _rel(out, ref) < (2e-6 if epi == ops.EPI_F32_ACCUM else 3e-3)
    small = ops.gemm(a[:256].to(dev), w.to(dev), b.to(dev), epi, resid=None if rd is None else rd[:256].contiguous())
    assert torch.equal(small, out[:256])


@pytest.mark.parametrize("epi", [ops.EPI_BF16_GELU, ops.EPI_F32_ACCUM])
def test_gemm_every_tile_shape_gives_the_same_bits(dev, epi):
    """m3_gemm_set_tile forces the dispatcher (diagnostic hook): the 64-, 128-, 192- and 256-wide kernels accumulate K in
    the same order, so one problem gives identical bits whichever of them runs it - the property that makes a pair's
    result independent of the batch it travels in and of the rank it lands on."""
    from mast3r_slam import _ffi
    L = _ffi.lib()
    m, n, k = 2048, 768, 1024
    g = torch.Generator(device="cpu").manual_seed(23 + epi)
    a = torch.randn(m, k, generator=g).bfloat16().to(dev)
    w = (torch.randn(n, k, generator=g) * 0.05).bfloat16().to(dev)
    b = torch.randn(n, generator=g).to(dev)
    r = torch.randn(m, n, generator=g).to(dev) if epi == ops.EPI_F32_ACCUM else None
    outs = {}
    prev = L.m3_gemm_set_tile(0)
    try:
        for tile in (64, 128, 192, 256):
            L.m3_gemm_set_tile(tile)
            assert L.m3_gemm_pick_tile(m, n, 1) == tile
            outs[tile] = ops.gemm(a, w, b, epi, resid=r)
    finally:
        L.m3_gemm_set_tile(prev)
    for tile in (128, 192, 256):
        assert torch.equal(outs[tile], outs[64]), tile


def test_conv_splitk_is_batch_invariant(dev):
    """A 16x16 map with K = 9*256 takes the split-K path (fp32 partial planes, fixed-order sum, epilogue in
    the finishing kernel).  The slice count depends on the per-image geometry only, so an image gives the
    same bits alone and inside a batch, and the result matches the fp32 reference."""
    from mast3r_slam import _ffi
    L = _ffi.lib()
    assert L.m3_conv3x3_splitk_bytes(1, 16, 16, 256, 256, 1) == 9 * 256 * 256 * 4        # 4 tiles, 36 K-tiles -> 9 slices
    assert L.m3_conv3x3_splitk_bytes(8, 16, 16, 256, 256, 1) == 8 * 9 * 256 * 256 * 4    # same slices for any batch
    assert L.m3_conv3x3_splitk_bytes(8, 128, 128, 256, 256, 1) == 0                      # fills the chip: direct
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.randn(3, 16, 16, 256, generator=g).bfloat16()
    w = (torch.randn(256, 3, 3, 256, generator=g) * 0.03).bfloat16()
    b = torch.randn(256, generator=g)
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), b, padding=1).permute(0, 2, 3, 1)
    out = ops.conv3x3(x.to(dev), w.to(dev), b.to(dev), ops.EPI_F32)
    assert _rel(out, ref) < 2e-6
    one = ops.conv3x3(x[1:2].to(dev), w.to(dev), b.to(dev), ops.EPI_F32)
    assert torch.equal(one[0], out[1])


@pytest.mark.parametrize("dt", DT16)
def test_conv_sliced_single_pass_equals_splitk_planes(dev, dt):
    """32 x 32 maps with K = 9 * 256 are a split-K geometry (4 slices per image, by the per-image rule).  A batch that
    already gives every CU an output tile (2 x 8 maps: 256 tiles) runs them as ONE pass in which a workgroup walks the 4
    slices itself and adds the slice sums in the finishing kernel's order; a single image still writes partial planes and
    runs k_splitk_finish.  Both must return the same bits for every image, for the plain, ReLU (+ input ReLU) and
    residual-add epilogues - the invariant "a pair gives the same bits alone or in a batch" on the small DPT maps."""
    from mast3r_slam import _ffi
    assert int(_ffi.lib().m3_conv3x3_splitk_bytes(1, 32, 32, 256, 256, 1)) == 4 * 1024 * 256 * 4
    g = torch.Generator(device="cpu").manual_seed(77)
    x = torch.randn(2, 8, 32, 32, 256, generator=g).to(dt).to(dev)
    wc = [(torch.randn(256, 3, 3, 256, generator=g) * 0.03).to(dt).to(dev) for _ in range(2)]
    bc = [(torch.randn(256, generator=g) * 0.1).to(dev) for _ in range(2)]
    res = torch.randn(2, 8, 32, 32, 256, generator=g).to(dt).to(dev)
    for epi, r, relu_in in ((ops.EPI_BF16, None, False), (ops.EPI_BF16_RELU, None, True), (ops.EPI_BF16_ADD, res, False)):
        both = ops.conv3x3_grouped2(x, wc[0], wc[1], bc[0], bc[1], epi, resid=r, relu_input=relu_in)       # 256 tiles: one sliced pass
        for v in range(2):
            for b in (0, 5):
                one = ops.conv3x3(x[v, b:b + 1], wc[v], bc[v], epi, resid=None if r is None else r[v, b:b + 1], relu_input=relu_in)
                assert torch.equal(both[v, b], one[0]), (epi, v, b, _rel(both[v, b], one[0]))
    ref = F.conv2d(x[0].float().permute(0, 3, 1, 2), wc[0].float().permute(0, 3, 1, 2), bc[0], padding=1).permute(0, 2, 3, 1)
    assert _rel(ops.conv3x3_grouped2(x, wc[0], wc[1], bc[0], bc[1], ops.EPI_BF16)[0], ref) < TOL16[dt]


def test_gemm_layout_identity_asymmetric(dev):
    """A = I with an asymmetric W catches a transposed C write (guide: 'A=I-check with ASYMMETRIC B')."""
    eye = torch.eye(128, device=dev).bfloat16()
    w = (torch.arange(128 * 128, device=dev).reshape(128, 128) % 251).float().bfloat16()
    assert torch.equal(ops.gemm(eye, w, None, ops.EPI_F32), w.float().T)


def test_gemm_rejects_bad_k(dev):
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.gemm(torch.zeros(128, 96, device=dev).bfloat16(), torch.zeros(128, 96, device=dev).bfloat16())


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("cfg", [(2, 16, 16, 64, 128, 1), (1, 32, 32, 256, 256, 1), (1, 32, 32, 128, 64, 2),
                                 (1, 20, 28, 64, 36, 1), (2, 128, 128, 64, 256, 1)])       # last: 256-row ping-pong conv
def test_conv3x3_implicit_gemm(dev, cfg, dt):
    b, h, w_, cin, cout, s = cfg
    g = torch.Generator().manual_seed(sum(cfg))
    x = torch.randn(b, h, w_, cin, generator=g).to(dt)
    w = (torch.randn(cout, 3, 3, cin, generator=g) * 0.05).to(dt)
    bias = torch.randn(cout, generator=g)
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), bias, stride=s, padding=1).permute(0, 2, 3, 1)
    out = ops.conv3x3(x.to(dev), w.to(dev), bias.to(dev), ops.EPI_F32, stride=s)
    assert tuple(out.shape) == tuple(ref.shape) and _rel(out, ref) < 2e-6
    res = torch.randn(ref.shape, generator=g).to(dt)
    out = ops.conv3x3(x.to(dev), w.to(dev), bias.to(dev), ops.EPI_BF16_ADD, stride=s, resid=res.to(dev))
    assert out.dtype == dt and _rel(out, ref + res.float()) < TOL16[dt]


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("cross", [False, True])
def test_attention_vs_softmax_reference(dev, cross, dt):
    b, h, t = 2, 3, 256
    g = torch.Generator().manual_seed(7)
    c = h * 64
    qkv = torch.randn(b * t, 3 * c, generator=g).to(dt)
    qkv[5, :64] *= 30.0                                           # a spiked query: exercises the running-max rescale
    out = torch.empty(b * t, c, dtype=dt, device=dev)
    d = qkv.to(dev)
    ops.attention(d, d[:, c:], d[:, 2 * c:], out, nbatch=b, heads=h, tq=t, tk=t, q_row_stride=3 * c,
                  kv_row_stride=3 * c, o_row_stride=c, q_batch_stride=t * 3 * c, kv_batch_stride=t * 3 * c,
                  o_batch_stride=t * c, kv_batch_shift=1 if cross else 0)
    q = qkv[:, :c].float().view(b, t, h, 64).transpose(1, 2)
    k = qkv[:, c:2 * c].float().view(b, t, h, 64).transpose(1, 2)
    v = qkv[:, 2 * c:].float().view(b, t, h, 64).transpose(1, 2)
    if cross:
        k, v = k.roll(-1, 0), v.roll(-1, 0)                      # batch item i attends item (i+1) % b
    ref = (torch.softmax(q @ k.transpose(-1, -2) * 0.125, -1) @ v).transpose(1, 2).reshape(b * t, c)
    assert _rel(out, ref) < (4e-3 if dt == torch.bfloat16 else 6e-4)     # P and O are 16-bit
    assert torch.isfinite(out).all()


@pytest.mark.parametrize("tq_tk_b_h", [(672, 672, 2, 16), (576, 576, 16, 12), (196, 196, 1, 2), (200, 150, 2, 3),
                                       (1, 1, 1, 1), (65, 129, 1, 2)])
def test_attention_ragged_token_counts(dev, tq_tk_b_h):
    """Token counts that are not multiples of the 64-key tile / 64- or 128-row query block: 512x336 -> 672,
    512x288 -> 576, 224x224 -> 196 (what resize_img emits, mast3r_utils.py:132-207), and tiny ragged cases.
    Key tail masked with -inf, query tail rows not stored: rows past Tq of a padded output buffer stay untouched."""
    tq, tk, b, h = tq_tk_b_h
    g = torch.Generator().manual_seed(tq + tk)
    c = h * 64
    q = torch.randn(b, tq, c, generator=g).bfloat16()
    kv = torch.randn(b, tk, 2 * c, generator=g).bfloat16()
    out = torch.full((b, tq + 3, c), 7.0, dtype=torch.bfloat16, device=dev)        # 3 guard rows per batch item
    qd, kvd = q.to(dev), kv.to(dev)
    ops.attention(qd, kvd, kvd[..., c:], out, nbatch=b, heads=h, tq=tq, tk=tk, q_row_stride=c, kv_row_stride=2 * c,
                  o_row_stride=c, q_batch_stride=tq * c, kv_batch_stride=tk * 2 * c, o_batch_stride=(tq + 3) * c)
    qf = q.float().view(b, tq, h, 64).transpose(1, 2)
    kf = kv[..., :c].float().view(b, tk, h, 64).transpose(1, 2)
    vf = kv[..., c:].float().view(b, tk, h, 64).transpose(1, 2)
    ref = (torch.softmax(qf @ kf.transpose(-1, -2) * 0.125, -1) @ vf).transpose(1, 2).reshape(b, tq, c)
    assert _rel(out[:, :tq], ref) < 4e-3
    assert bool((out[:, tq:] == 7.0).all())


def test_rope2d_layernorm_and_elementwise(dev):
    g = torch.Generator().manual_seed(3)
    gh, gw, heads = 8, 16, 4
    t = gh * gw
    x = torch.randn(2 * t, heads * 64, generator=g).bfloat16()
    pos = OM.patch_positions(gh * 16, gw * 16)
    cos, sin = OM.rope_tables(17)
    ref = OM.rope2d(x.float().view(2, t, heads, 64).transpose(1, 2), pos, cos, sin).transpose(1, 2).reshape(2 * t, -1)
    cs = torch.stack([cos, sin], -1).to(dev).contiguous()
    xd = x.to(dev).clone()
    ops.rope2d_(xd, pos.to(torch.int32).to(dev), cs, row_stride=heads * 64, tokens=2 * t, heads=heads, tokens_per_image=t)
    assert _rel(xd, ref) < 3e-3
    # LayerNorm (C = 768 and 1024)
    for c in (768, 1024):
        xf = torch.randn(37, c, generator=g) * 3 + 1
        gm, bt = torch.randn(c, generator=g), torch.randn(c, generator=g)
        out = ops.layernorm(xf.to(dev), gm.to(dev), bt.to(dev))
        assert _rel(out, F.layer_norm(xf, (c,), gm, bt, 1e-6)) < 3e-3
    # bilinear x2 align_corners, un-shuffle, concat, relu, add
    y = torch.randn(2, 5, 7, 16, generator=g).bfloat16()
    ref = F.interpolate(y.float().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    assert _rel(ops.upsample2x(y.to(dev)), ref) < 3e-3
    z = torch.randn(2 * 3 * 4, 4 * 8, generator=g).bfloat16()    # s=2, C=8
    un = ops.unshuffle(z.to(dev), 2, 3, 4, 2, 8, 16).cpu()
    ref = z.view(2, 3, 4, 2, 2, 8).permute(0, 1, 3, 2, 4, 5).reshape(2, 6, 8, 8)
    assert torch.equal(un[..., :8], ref) and bool((un[..., 8:] == 0).all())
    a, b = torch.randn(9, 16, generator=g).bfloat16(), torch.randn(9, 24, generator=g).bfloat16()
    assert torch.equal(ops.concat2(a.to(dev), b.to(dev)).cpu(), torch.cat([a, b], 1))
    r = torch.randn(64, generator=g).bfloat16()
    assert torch.equal(ops.relu(r.to(dev)).cpu(), torch.relu(r))
    assert torch.equal(ops.add(r.to(dev), r.to(dev)).cpu(), (r.float() * 2).bfloat16())


def test_fp16_storage_variants_of_the_elementwise_ops(dev):
    """The *_dt entry points with dtype = M3_DT_F16: LayerNorm / cast outputs, upsample, add, ReLU (sign bit),
    bf16 <-> fp16 cast, patchify and the descriptor post-processing read."""
    g = torch.Generator().manual_seed(4)
    xf = torch.randn(37, 768, generator=g) * 3 + 1
    gm, bt = torch.randn(768, generator=g), torch.randn(768, generator=g)
    out = ops.layernorm(xf.to(dev), gm.to(dev), bt.to(dev), dtype=torch.float16)
    assert out.dtype == torch.float16 and _rel(out, F.layer_norm(xf, (768,), gm, bt, 1e-6)) < 4e-4
    v = torch.randn(1000, generator=g) * 10
    assert torch.equal(ops.cast_f32(v.to(dev), torch.float16).cpu(), v.half())
    y = torch.randn(2, 5, 7, 16, generator=g).half()
    ref = F.interpolate(y.float().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    assert _rel(ops.upsample2x(y.to(dev)), ref) < 4e-4
    r = torch.randn(64, generator=g).half()
    assert torch.equal(ops.relu(r.to(dev)).cpu(), torch.relu(r))
    assert torch.equal(ops.add(r.to(dev), r.to(dev)).cpu(), (r.float() * 2).half())
    b16 = (torch.randn(4096, generator=g) * 5).bfloat16()
    assert torch.equal(ops.cast16(b16.to(dev), torch.float16).cpu(), b16.float().half())
    assert torch.equal(ops.cast16(b16.float().half().to(dev), torch.bfloat16).cpu(), b16.float().half().float().bfloat16())
    img = torch.randint(0, 256, (1, 32, 48, 3), generator=g, dtype=torch.uint8)
    pa = ops.patchify16(img.to(dev), torch.float16)
    x = ((img.float() / 255.0 - 0.5) / 0.5).permute(0, 3, 1, 2)
    assert torch.equal(pa.cpu(), F.unfold(x, kernel_size=16, stride=16).transpose(1, 2).reshape(-1, 768).half())
    f = torch.randn(2 * 1 * 2, 6400, generator=g).half()
    desc, dconf = ops.desc_post(f.to(dev), 2, 16, 32)
    ps = F.pixel_shuffle(f.float().view(2, 2, 6400).transpose(1, 2).reshape(2, 6400, 1, 2), 16).permute(0, 2, 3, 1)
    assert _rel(desc, ps[..., :24] / ps[..., :24].norm(dim=-1, keepdim=True)) < 1e-6
    desc16, dconf16 = ops.desc_post(f.to(dev), 2, 16, 32, torch.float16)      # "fp16 features": one rounding of the fp32 value
    assert desc16.dtype == torch.float16 and torch.equal(desc16, desc.half()) and torch.equal(dconf16, dconf)
    with pytest.raises(TypeError, match="mixed 16-bit"):
        ops.add(r.to(dev), r.bfloat16().to(dev))


@pytest.mark.parametrize("dt", DT16)
def test_fused_head_tail_matches_unfused_chain(dev, dt):
    """conv3x3+ReLU -> 1x1 (4 ch) -> pts_post in one launch.  The fused kernel keeps the 128-channel ReLU map in
    fp32 registers (never rounded to 16 bits), so it matches a plain torch fp32 reference to fp32 accuracy; the
    three separate ops round that map once and agree to the 16-bit rounding."""
    g = torch.Generator(device="cpu").manual_seed(21)
    b, h, w, cin = 1, 50, 120, 64                                            # ragged: 6000 pixels (no split-K at this size)
    x = torch.randn(b, h, w, cin, generator=g).to(dt)
    wc = (torch.randn(128, 3, 3, cin, generator=g) * 0.05).to(dt)
    bc = torch.randn(128, generator=g) * 0.1
    w4 = (torch.randn(4, 128, generator=g) * 0.05).to(dt)
    b4 = torch.randn(4, generator=g) * 0.1
    d = lambda t: t.to(dev)
    pts, conf = ops.conv3x3_relu_head4(d(x), d(wc), d(bc), d(w4), d(b4))
    h2 = ops.conv3x3(d(x), d(wc), d(bc), ops.EPI_BF16_RELU)
    raw = ops.gemm(h2.view(-1, 128), d(w4), d(b4), ops.EPI_F32)
    pts_u, conf_u = ops.pts_post(raw.view(b, h, w, 4))
    assert _rel(pts, pts_u) < TOL16[dt] and _rel(conf, conf_u) < TOL16[dt]
    y = torch.relu(F.conv2d(x.float().permute(0, 3, 1, 2), wc.float().permute(0, 3, 1, 2), bc, padding=1)).permute(0, 2, 3, 1)
    r = y @ w4.float().T + b4
    dn = r[..., :3].norm(dim=-1, keepdim=True)
    assert _rel(pts, r[..., :3] / dn.clip(min=1e-8) * torch.expm1(dn)) < 5e-6      # fp32 accumulation order only
    assert _rel(conf, 1 + torch.exp(r[..., 3])) < 5e-6


@pytest.mark.parametrize("shape", [(1024, 768, 256), (16384, 768, 128)])       # 64/128-tile path and the 256x192 path
def test_grouped_launches_equal_separate_ops(dev, shape):
    """The 2-group GEMM / LayerNorm launches of the decoder (one launch for both branches) give the same bits
    as two separate single-group calls; swap=True normalises the OTHER branch's rows (norm_y)."""
    m, n, k = shape
    g = torch.Generator(device="cpu").manual_seed(m + n)
    a = torch.randn(2, m, k, generator=g).bfloat16().to(dev)
    w = [(torch.randn(n, k, generator=g) * 0.05).bfloat16().to(dev) for _ in range(2)]
    b = [torch.randn(n, generator=g).to(dev) for _ in range(2)]
    r = torch.randn(2, m, n, generator=g).to(dev)
    for epi in (ops.EPI_BF16, ops.EPI_BF16_GELU, ops.EPI_F32_ACCUM):
        res = r.clone() if epi == ops.EPI_F32_ACCUM else None
        both = ops.gemm_grouped2(a, w[0], w[1], b[0], b[1], epi, resid=res)
        for v in range(2):
            one = ops.gemm(a[v], w[v], b[v], epi, resid=None if res is None else r[v].contiguous())
            assert torch.equal(both[v], one)
    x = torch.randn(2, 512, 768, generator=g).to(dev) * 3 + 1
    gam = [torch.randn(768, generator=g).to(dev) for _ in range(2)]
    bet = [torch.randn(768, generator=g).to(dev) for _ in range(2)]
    y = ops.layernorm_grouped2(x, gam[0], bet[0], gam[1], bet[1])
    ys = ops.layernorm_grouped2(x, gam[0], bet[0], gam[1], bet[1], swap=True)
    for v in range(2):
        assert torch.equal(y[v], ops.layernorm(x[v].contiguous(), gam[v], bet[v]))
        assert torch.equal(ys[v], ops.layernorm(x[1 - v].contiguous(), gam[v], bet[v]))     # group v's params on the other rows
        ref = F.layer_norm(x[v].cpu(), (768,), gam[v].cpu(), bet[v].cpu(), 1e-6)
        assert _rel(y[v], ref) < 3e-3


def test_patchify_and_cast(dev):
    """uint8 NHWC image -> [tokens, 16*16*3] bf16 patch rows with the (x/255 - 0.5)/0.5 normalisation, in the
    (c, dy, dx) order of a Conv2d(3, E, 16, 16) weight flattened to [E, 768]; fp32 -> bf16 cast is RNE."""
    g = torch.Generator(device="cpu").manual_seed(2)
    img = torch.randint(0, 256, (2, 32, 48, 3), generator=g, dtype=torch.uint8)
    out = ops.patchify16(img.to(dev)).float().cpu()
    x = ((img.float() / 255.0 - 0.5) / 0.5).permute(0, 3, 1, 2)                       # NCHW
    ref = F.unfold(x, kernel_size=16, stride=16).transpose(1, 2).reshape(-1, 768)     # rows = tokens, cols = (c, dy, dx)
    assert out.shape == ref.shape and _rel(out, ref) < 3e-3
    v = torch.randn(1000, generator=g) * 10
    assert torch.equal(ops.f32_to_bf16(v.to(dev)).cpu(), v.bfloat16())
    # a contiguous uint8 view at an odd storage offset (round-3 advisor finding: k_patchify's 8-byte loads): the C entry
    # point answers with a status, the wrapper re-aligns by copying - same result either way
    buf = torch.zeros(img.numel() + 16, dtype=torch.uint8, device=dev)
    off = buf[3:3 + img.numel()].view(img.shape)
    off.copy_(img.to(dev))
    assert off.data_ptr() % 8 != 0 and off.is_contiguous()
    from mast3r_slam import _ffi
    dst = torch.empty((2 * 2 * 3, 768), dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError):
        _ffi.call("m3_patchify16_dt", _ffi.ptr(off), _ffi.ptr(dst), 2, 32, 48, 0, _ffi.stream_ptr())
    assert torch.equal(ops.patchify16(off).float().cpu(), out)


def test_heads_postprocessing(dev):
    g = torch.Generator().manual_seed(11)
    raw = torch.randn(2, 16, 16, 4, generator=g)
    pts, conf = ops.pts_post(raw.to(dev))
    d = raw[..., :3].norm(dim=-1, keepdim=True)
    assert _rel(pts, raw[..., :3] / d * torch.expm1(d)) < 1e-6 and _rel(conf, 1 + raw[..., 3].exp()) < 1e-6
    f = torch.randn(2 * 1 * 2, 6400, generator=g).bfloat16()      # B=2, 16x32 image
    desc, dconf = ops.desc_post(f.to(dev), 2, 16, 32)
    ps = F.pixel_shuffle(f.float().view(2, 2, 6400).transpose(1, 2).reshape(2, 6400, 1, 2), 16).permute(0, 2, 3, 1)
    assert _rel(desc, ps[..., :24] / ps[..., :24].norm(dim=-1, keepdim=True)) < 1e-6
    assert _rel(dconf, ps[..., 24].exp()) < 1e-6


@pytest.fixture(scope="module")
def tiny(dev):
    cfg = M.TINY_CFG
    w = M.init_random_weights(cfg, seed=1)
    return cfg, w, M.Mast3rFull(weights=w, cfg=cfg, device=dev)


def test_two_view_network_vs_cpu_oracle(tiny, dev):
    """Same structure as the full model (2 encoder + 4 decoder blocks, DPT + feature heads) on 128x256
    images, 2 pairs: pointmaps within 1e-3 rel-L2 of the fp32 oracle (BASELINE target), descriptors
    within 6e-3 (the feature MLP output is stored in bf16)."""
    cfg, w, net = tiny
    h, wd = 128, 256
    im1 = np.stack([synthetic.textured_image(h, wd, s) for s in (0, 2)])
    im2 = np.stack([synthetic.textured_image(h, wd, s) for s in (1, 3)])
    o1, o2 = net.reconstruct_batch(im1, im2)
    r1, r2 = OM.reconstruct(w, torch.from_numpy(im1), torch.from_numpy(im2), cfg)
    for o, r in ((o1, r1), (o2, r2)):
        assert o["pts3d"].shape == (2, h, wd, 3) and o["desc"].shape == (2, h, wd, 24)
        assert _rel(o["pts3d"], r["pts3d"]) < 1e-3
        assert _rel(o["conf"], r["conf"]) < 1e-4
        assert _rel(o["desc"], r["desc"]) < 6e-3
        assert _rel(o["desc_conf"], r["desc_conf"]) < 6e-3
        assert float((o["desc"].norm(dim=-1) - 1).abs().max()) < 1e-5
    # batched == per-pair (pairs are independent units: the sharding invariant)
    s1, s2 = net.reconstruct_batch(im1[1:], im2[1:])
    assert torch.equal(s1["pts3d"][0], o1["pts3d"][1]) and torch.equal(s2["desc"][0], o2["desc"][1])


def test_width_without_fold_statistics_keeps_the_layernorm_kernels(dev):
    """The LayerNorm fold needs a canonical sum tree for the stream width (m3_ln_slot_count > 0: 768, 1024).  An fp16 model of
    another width (encoder 1280) must build with the fold off - for BOTH streams, the decoder's 768 included - and run the
    LayerNorm kernels: one forward against the fp32 oracle, the tolerances of test_two_view_network_vs_cpu_oracle."""
    from mast3r_slam import _ffi
    assert int(_ffi.lib().m3_ln_slot_count(2, 1280, 1)) == 0 and int(_ffi.lib().m3_ln_slot_count(2, 1536, 2)) == 0
    assert int(_ffi.lib().m3_ln_slot_count(2, 768, 2)) > 0
    cfg = dict(M.TINY_CFG, enc_dim=1280, enc_heads=20)
    w = M.init_random_weights(cfg, seed=3)
    net = M.Mast3rFull(weights=w, cfg=cfg, device=dev, precision="fp16")
    assert net.ln_fold is False and not any(k.endswith(".fw") for k in net.P)
    assert M.Mast3rFull(weights=M.init_random_weights(M.TINY_CFG, seed=1), cfg=M.TINY_CFG, device=dev, precision="fp16").ln_fold is True
    h, wd = 128, 256
    im1, im2 = synthetic.textured_image(h, wd, 0)[None], synthetic.textured_image(h, wd, 1)[None]
    o1, o2 = net.reconstruct_batch(im1, im2)
    r1, r2 = OM.reconstruct(w, torch.from_numpy(im1), torch.from_numpy(im2), cfg)
    for o, r in ((o1, r1), (o2, r2)):
        assert _rel(o["pts3d"], r["pts3d"]) < 1e-3
        assert _rel(o["conf"], r["conf"]) < 1e-4
        assert _rel(o["desc"], r["desc"]) < 6e-3
        assert _rel(o["desc_conf"], r["desc_conf"]) < 6e-3


@pytest.mark.parametrize("precision,ln_fold", [("fp16", None), ("bf16", None), ("fp16", "0")])
def test_trunk_launches_follow_the_stream_form(dev, monkeypatch, precision, ln_fold):
    """Which entry points one encoder + decoder pass issues, counted from the structure (E encoder blocks of 4 GEMMs and one
    attention, D two-group decoder blocks of 7 GEMMs and two attentions, the two embeddings, the hooks).  Every parity test
    passes at its tolerance on either form of the residual stream, so only this pins that the fp16 trunk runs the LayerNorm
    fold (no LayerNorm launch but enc_norm / dec_norm on the hi / lo planes, mid-depth taps are copies of the hi plane) and
    that the bf16 trunk and M3_LN_FOLD=0 run the LayerNorm kernels: norm1 + norm_y of a decoder block from ONE dual2 launch."""
    from mast3r_slam import _ffi
    if ln_fold is not None:
        monkeypatch.setenv("M3_LN_FOLD", ln_fold)
    cfg = M.TINY_CFG
    net = M.Mast3rFull(weights=M.init_random_weights(cfg, seed=1), cfg=cfg, device=dev, precision=precision)
    h, wd = 128, 256                                                 # 128 tokens per image: an even row count
    im1, im2 = (net._as_images(synthetic.textured_image(h, wd, s)) for s in (0, 1))
    counts, real = {}, _ffi.call

    def counting(name, *args):
        counts[name] = counts.get(name, 0) + 1
        return real(name, *args)

    monkeypatch.setattr(_ffi, "call", counting)
    tok, grid = net.encode_tokens(im1, im2)
    m = grid[0] * grid[1]
    taps = net.decode_tokens(tok[:m], tok[m:], 1, grid)
    assert len(taps[0]) == len(taps[1]) == len(cfg["hooks"])
    E, D, hooks = cfg["enc_depth"], cfg["dec_depth"], cfg["hooks"]
    last, mid = int(D in hooks), sum(1 for k in hooks if 0 < k < D)
    folded = precision == "fp16" and ln_fold is None
    assert net.ln_fold is folded
    want = {"m3_gemm_ex": (1 + 4 * E) + (1 + 7 * D), "m3_attention_prescaled_dt": E + 2 * D}
    if folded:
        want.update(m3_layernorm_hl_dt=1 + last, m3_layernorm_dt=0, m3_layernorm_dual2_dt=0, m3_layernorm_grouped2_dt=0)
        taps_cast = 0 if net.hdt == net.tdt else mid                 # a mid-depth tap is a copy of the hi plane when the types agree
    else:
        want.update(m3_layernorm_hl_dt=0, m3_layernorm_dt=2 * E + 1, m3_layernorm_dual2_dt=D, m3_layernorm_grouped2_dt=2 * D + last)
        taps_cast = mid                                              # the fp32 stream is rounded (cast_f32) to the heads' type, whichever it is
    want.update(m3_cast_f32_dt=taps_cast, m3_cast16=0 if net.hdt == net.tdt else 1)     # tap 0: one cast of the encoder tokens
    assert {k: counts.get(k, 0) for k in want} == want


def test_graphed_reconstruct_equals_eager(tiny, dev):
    """The hipGraph-replayed network (fixed shape, static buffers) returns the same bits as eager launches,
    call after call with different images."""
    cfg, w, net = tiny
    h, wd = 128, 256
    g = net.graphed(1, h, wd)
    for seeds in ((0, 1), (5, 6)):
        im1 = synthetic.textured_image(h, wd, seeds[0])[None]
        im2 = synthetic.textured_image(h, wd, seeds[1])[None]
        e1, e2 = net.reconstruct_batch(im1, im2)
        o1, o2 = g(im1, im2)
        for k in ("pts3d", "conf", "desc", "desc_conf"):
            assert torch.equal(o1[k], e1[k]) and torch.equal(o2[k], e2[k])
    with pytest.raises(ValueError):
        g(np.zeros((1, 64, 256, 3), np.uint8), np.zeros((1, 64, 256, 3), np.uint8))


def test_operator_api_contract(tiny, dev):
    """Return tuples and shapes of the reference operator API (mast3r_utils.py:255-500)."""
    cfg, w, net = tiny
    h, wd = 128, 256
    fi = create_frame(0, torch.from_numpy(synthetic.textured_image(h, wd, 0)).to(dev))
    fj = create_frame(1, torch.from_numpy(synthetic.textured_image(h, wd, 1)).to(dev))
    Xii, Cii, feat, pos = mast3r_utils.mast3r_inference_mono(net, fi)
    n, t = h * wd, (h // 16) * (wd // 16)
    assert Xii.shape == (n, 3) and Cii.shape == (n, 1) and feat.shape == (t, 1024) and pos.shape == (t, 2)
    X, C, D, Q = mast3r_utils.mast3r_asymmetric_inference(net, fi, fj)
    assert X.shape == (2, h, wd, 3) and C.shape == (2, h, wd) and D.shape == (2, h, wd, 24) and Q.shape == (2, h, wd)
    X4, C4, D4, Q4 = mast3r_utils.mast3r_symmetric_inference(net, fi, fj)
    assert X4.shape == (4, h, wd, 3) and Q4.shape == (4, h, wd)
    assert torch.equal(X4[0], X[0]) and torch.equal(X4[1], X[1])      # (ii, ji) agree with the asymmetric call
    out = mast3r_utils.mast3r_match_asymmetric(net, fi, fj)
    assert len(out) == 8
    idx, valid, Xi, Ci, Qi, Xj, Cj, Qj = out
    assert idx.shape == (1, n) and valid.shape == (1, n, 1) and valid.dtype == torch.bool
    assert Xi.shape == (1, n, 3) and Ci.shape == (1, n, 1) and Qj.shape == (1, n, 1)
    feats = torch.stack([fi.feat, fj.feat])
    shp = [torch.tensor([[h, wd]])] * 2
    sym = mast3r_utils.mast3r_match_symmetric(net, feats, None, feats.flip(0), None, shp, shp)
    assert len(sym) == 8 and sym[0].shape == (2, n) and sym[2].shape == (2, n, 1) and sym[4].shape == (2, n, 1)
    Xs, Cs, Ds, Qs = mast3r_utils.mast3r_decode_symmetric_batch(net, feats, None, feats.flip(0), None, shp, shp)
    assert Xs.shape == (4, 2, h, wd, 3)
    assert _rel(Xs[0, 0], X[0]) < 1e-6                                 # same decode, batched with others
    with pytest.raises(NotImplementedError):
        mast3r_utils.load_mast3r("dunemast3r")


@pytest.mark.parametrize("m_n_k", [(256, 192, 64), (2048, 3072, 1024), (16384, 768, 64)])   # 128 / 256x256 / 256x192 tiles
def test_gemm_with_fused_rope_epilogue(dev, m_n_k):
    m, n, k = m_n_k
    g = torch.Generator().manual_seed(m)
    gh, gw = 8, 16
    t = gh * gw
    a = torch.randn(m, k, generator=g).bfloat16()
    w = (torch.randn(n, k, generator=g) * 0.05).bfloat16()
    b = torch.randn(n, generator=g)
    rope_cols = n // 64 // 3 * 2 * 64                              # first two thirds are q|k heads
    pos = OM.patch_positions(gh * 16, gw * 16)
    cos, sin = OM.rope_tables(17)
    ref = a.float() @ w.float().T + b
    heads = rope_cols // 64
    rot = OM.rope2d(ref[:, :rope_cols].reshape(m // t, t, heads, 64).transpose(1, 2), pos, cos, sin)
    ref = torch.cat([rot.transpose(1, 2).reshape(m, rope_cols), ref[:, rope_cols:]], 1)
    # cos/sin computed in the epilogue from the tokens' grid positions (hardware sin/cos, ~1e-6 absolute)
    out_p = ops.gemm_rope(a.to(dev), w.to(dev), b.to(dev), pos.to(torch.int32).to(dev).contiguous(), rope_cols)
    assert _rel(out_p, ref) < 3e-3
    with pytest.raises(TypeError, match="int32"):                   # positions only: an f32 coefficient table is refused
        ops.gemm_rope(a.to(dev), w.to(dev), b.to(dev), torch.zeros(t, 2, 2, 16, device=dev), rope_cols)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_rope_lds_table_returns_the_per_element_bits(dev, dtype):
    """ops.rope_bound (m3_gemm_desc.rope_max_pos): with the positions' range promised, every workgroup builds the cos / sin of
    all (position, frequency) pairs once in LDS; the rotation must return the bits of the per-element v_sin / v_cos form, in
    every tile shape (64 / 128 / 192 / 256), for one and two groups, with and without bf16 v columns; a bound the table cannot
    hold (> 64) and a missing promise fall back to the per-element form."""
    gh, gw = 12, 20
    t = gh * gw
    m, k = 8 * t, 128
    g = torch.Generator().manual_seed(31)
    gy, gx = torch.meshgrid(torch.arange(gh), torch.arange(gw), indexing="ij")
    mk_pos = lambda: torch.stack([gy.reshape(-1), gx.reshape(-1)], -1).to(torch.int32).to(dev).contiguous()
    plain, bound, toobig = mk_pos(), ops.rope_bound(mk_pos(), max(gh, gw)), ops.rope_bound(mk_pos(), 65)
    a = torch.randn(2, m, k, generator=g).to(dtype).to(dev)
    prev = ops._ffi.lib().m3_gemm_set_tile(0)
    try:
        for tile in (64, 128, 192, 256):
            ops._ffi.lib().m3_gemm_set_tile(tile)
            for n, rc, qc in ((768, 512, 256), (1536, 1024, 512), (192, 192, 0)):
                w = [(torch.randn(n, k, generator=g) * 0.1).to(dtype).to(dev) for _ in range(2)]
                b = [torch.randn(n, generator=g).to(dev) for _ in range(2)]
                for pv in ((False, True) if dtype == torch.float16 and rc < n else (False,)):
                    one = lambda pos: ops.gemm_ex(a[0], w[0], b[0], ops.EPI_BF16_ROPE, rope=(pos, rc, qc, 0.25), pv_bf16=pv)
                    two = lambda pos: ops.gemm_ex(a, w[0], b[0], ops.EPI_BF16_ROPE, w1=w[1], bias1=b[1], rope=(pos, rc, qc, 0.25), pv_bf16=pv)
                    ref1, ref2 = one(plain), two(plain)
                    assert torch.equal(one(bound), ref1) and torch.equal(two(bound), ref2)
                    assert torch.equal(one(toobig), ref1)
                    assert torch.equal(ops.gemm_rope(a[0], w[0], b[0], bound, rc, qc, 0.25, pv_bf16=pv), ref1)     # the older entry points
                    assert torch.equal(ops.gemm_grouped2(a, w[0], w[1], b[0], b[1], ops.EPI_BF16_ROPE, rope=(bound, rc, qc, 0.25), pv_bf16=pv), ref2)
    finally:
        ops._ffi.lib().m3_gemm_set_tile(prev)
    # and the table form against the fp32 reference rotation
    pos = OM.patch_positions(gh * 16, gw * 16)
    cos, sin = OM.rope_tables(max(gh, gw) + 1)
    n, rc = 768, 512
    w0 = (torch.randn(n, k, generator=g) * 0.1).to(dtype)
    ref = a[0].float().cpu() @ w0.float().T
    rot = OM.rope2d(ref[:, :rc].reshape(m // t, t, rc // 64, 64).transpose(1, 2), pos, cos, sin)
    ref = torch.cat([rot.transpose(1, 2).reshape(m, rc), ref[:, rc:]], 1)
    out = ops.gemm_ex(a[0], w0.to(dev), None, ops.EPI_BF16_ROPE, rope=(bound, rc))
    assert _rel(out, ref) < (3e-3 if dtype == torch.bfloat16 else 4e-4)


def test_frame_tracker_end_to_end(tiny, dev):
    """The reference's per-frame flow (slam.py:159-214): mono-init a keyframe, then FrameTracker.track a new
    frame against it through the injected operator (tracker.py:51-175).  Random weights give meaningless
    geometry, so only the contract is checked: types, shapes, the relocalisation gate and pose bookkeeping."""
    from mast3r_slam import config
    from mast3r_slam.frame import Keyframes
    from mast3r_slam.tracker import FrameTracker
    cfg, w, net = tiny
    h, wd = 128, 256
    kf = create_frame(0, torch.from_numpy(synthetic.textured_image(h, wd, 0)).to(dev))
    X, C, feat, pos = mast3r_utils.mast3r_inference_mono(net, kf)
    kf.update_pointmap(X, C)
    keyframes = Keyframes()
    keyframes.append(kf)
    fr = create_frame(1, torch.from_numpy(synthetic.textured_image(h, wd, 1)).to(dev))
    tr = FrameTracker(net, keyframes)
    for simple in (True, False):
        # Q_conf / C_conf lowered so that the random-weight confidences pass the validity masks
        config.set_config({"matching": {"use_simple": simple, "dist_thresh": 1e9},
                           "tracking": {"Q_conf": -1.0, "C_conf": -1.0, "min_match_frac": 0.0}})
        try:
            tr.cfg = config.get_config()["tracking"]
            tr.reset_idx_f2k()
            n_before, pose_before = keyframes.last_keyframe().N, fr.T_WC.clone()
            new_kf, match_info, try_reloc = tr.track(fr, mast3r_match_fn=mast3r_utils.mast3r_match_asymmetric)
        finally:
            config.reset_config()
        status = float(tr.last_info.reshape(-1)[3])
        assert fr.T_WC.shape == (1, 8) and torch.isfinite(fr.T_WC).all()
        assert tr.idx_f2k is None or tr.idx_f2k.shape == (1, h * wd)
        if try_reloc:
            # random-weight pointmaps are not a consistent scene: the Gauss-Newton step can diverge, which the device solve
            # reports (status 2) and track() turns into the reference's `except` branch (tracker.py:139-141): relocalise,
            # frame pose and keyframe map untouched
            assert status == 2.0 and (new_kf, match_info) == (False, [])
            assert torch.equal(fr.T_WC, pose_before) and keyframes.last_keyframe().N == n_before
        else:
            assert status in (0.0, 1.0) and isinstance(new_kf, bool) and len(match_info) == 6
            assert keyframes.last_keyframe().N == n_before + 1              # keyframe pointmap was fused again
    # the min_match_frac gate (tracker.py:116-119): impossible thresholds -> relocalise
    config.set_config({"tracking": {"Q_conf": 1e9}})
    try:
        tr.cfg = config.get_config()["tracking"]
        assert tr.track(fr, mast3r_match_fn=mast3r_utils.mast3r_match_asymmetric) == (False, [], True)
    finally:
        config.reset_config()


def test_non_square_512x384_pair(tiny, dev):
    """BASELINE configs[0] image shape on the device path: 512x384 (T = 768 tokens) through network + matcher."""
    from mast3r_slam import config, matching
    cfg, w, net = tiny
    h, wd = 384, 512
    im1 = synthetic.textured_image(h, wd, 4)[None]
    im2 = synthetic.textured_image(h, wd, 5)[None]
    o1, o2 = net.reconstruct_batch(im1, im2)
    r1, r2 = OM.reconstruct(w, torch.from_numpy(im1), torch.from_numpy(im2), cfg)
    assert o1["pts3d"].shape == (1, h, wd, 3)
    assert _rel(o1["pts3d"], r1["pts3d"]) < 1e-3 and _rel(o2["pts3d"], r2["pts3d"]) < 1e-3
    config.set_config({"matching": {"use_simple": False}})
    try:
        idx, valid = matching.match(o1["pts3d"], o2["pts3d"], o1["desc"], o2["desc"])
    finally:
        config.reset_config()
    assert idx.shape == (1, h * wd) and valid.shape == (1, h * wd, 1)


@pytest.mark.parametrize("shape", [(1344, 3072, 1024), (672, 3072, 1024), (2688, 2304, 768)])
def test_small_tile_gemm_is_race_free_at_high_occupancy(dev, shape):
    """Regression for an LDS write-after-read race: the 64x64-tile kernel runs 4-5 workgroups
    per CU; its end-of-K-tile barrier used to be scheduled ahead of the wait for the wave's last fragment reads, so
    a neighbour could re-stage the buffer under them - 1-3 tiles per 1000 came out with one K-tile of stale rows
    (O(1) errors, different tiles every launch).  Every launch must reproduce bf16(fp32-epilogue result) exactly."""
    from mast3r_slam import _ffi
    m, n, k = shape
    g = torch.Generator(device="cpu").manual_seed(m)
    a = torch.randn(m, k, generator=g).bfloat16().to(dev)
    w = (torch.randn(n, k, generator=g) * 0.05).bfloat16().to(dev)
    b = torch.randn(n, generator=g).to(dev)
    assert _ffi.lib().m3_gemm_pick_tile(m, n, 1) in (64, 128)          # the small-problem kernel (2-5 workgroups per CU)
    want = ops.gemm(a, w, b, ops.EPI_F32).bfloat16()
    for run in range(12):
        out = ops.gemm(a, w, b, ops.EPI_BF16)
        bad = int((out != want).sum())
        assert bad == 0, f"launch {run}: {bad} elements differ"


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("upsample", [False, True])
@pytest.mark.parametrize("bhw", [(2, 32, 48), (1, 64, 64), (3, 16, 16), (1, 48, 80)])
def test_dpt_tail_direct_convolution(dev, dt, upsample, bhw):
    """m3_dpt_tail_grouped2_dt (x2 upsample fused into the LDS halo staging + conv3x3 + ReLU + 1x1 + pointmap post-processing)
    against the separate operators (k_upsample2x -> m3_conv3x3_relu_head4_dt: same 16-bit rounding of the upsampled map,
    fp32 summation order differs) and against a plain torch fp32 chain."""
    b, h, w = bhw                                                     # OUTPUT size
    g = torch.Generator(device="cpu").manual_seed(h * 7 + w + int(upsample))
    ih, iw = (h // 2, w // 2) if upsample else (h, w)
    x = torch.randn(b, ih, iw, 128, generator=g).to(dt)
    wc = (torch.randn(128, 3, 3, 128, generator=g) * 0.03).to(dt)
    bc = torch.randn(128, generator=g) * 0.1
    w4 = (torch.randn(4, 128, generator=g) * 0.05).to(dt)
    b4 = torch.randn(4, generator=g) * 0.1
    d = lambda t: t.to(dev)
    pts, conf = ops.dpt_tail(d(x), d(wc), d(bc), d(w4), d(b4), upsample=upsample)
    assert pts.shape == (b, h, w, 3) and conf.shape == (b, h, w)
    xu = ops.upsample2x(d(x)) if upsample else d(x)
    pts_u, conf_u = ops.conv3x3_relu_head4(xu, d(wc), d(bc), d(w4), d(b4))
    # same arithmetic; with the upsample, FMA contraction may round a few interpolated values to the neighbouring 16-bit number
    tol_u = 0.2 * TOL16[dt] if upsample else 5e-6
    assert _rel(pts, pts_u) < tol_u and _rel(conf, conf_u) < tol_u
    xf = x.float().permute(0, 3, 1, 2)
    if upsample:
        xf = F.interpolate(xf, scale_factor=2, mode="bilinear", align_corners=True)
    y = torch.relu(F.conv2d(xf, wc.float().permute(0, 3, 1, 2), bc, padding=1)).permute(0, 2, 3, 1)
    r = y @ w4.float().T + b4
    dn = r[..., :3].norm(dim=-1, keepdim=True)
    tol = 5e-6 if not upsample else TOL16[dt]                          # the interpolated map is rounded to 16 bits once
    assert _rel(pts, r[..., :3] / dn.clip(min=1e-8) * torch.expm1(dn)) < tol
    assert _rel(conf, 1 + torch.exp(r[..., 3])) < tol


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("bhw_c", [(16, 128, 128, 256), (2, 64, 64, 256), (2, 16, 16, 256), (1, 50, 72, 64)])
def test_conv3x3_with_relu_on_its_input_fragments(dev, dt, bhw_c):
    """M3_EPI_INPUT_RELU (the DPT residual unit's relu(x) -> conv1): the ReLU is applied to the operand fragments in
    registers (signed 16-bit max with 0), relu(x) is never written.  Must equal conv3x3(relu(x)) bit for bit on every
    kernel the dispatcher picks: 256-row tiles (16 x 128 x 128), 128-row tiles, split-K (16 x 16 maps) and a ragged size;
    single and 2-group launches; negative zeros and padding included."""
    b, h, w, c = bhw_c
    g = torch.Generator(device="cpu").manual_seed(h + w + c)
    x = torch.randn(2, b, h, w, c, generator=g).to(dt)
    x[0, 0, 0, 0, :8] = -0.0
    wc = [(torch.randn(256, 3, 3, c, generator=g) * 0.03).to(dt).to(dev) for _ in range(2)]
    bc = [torch.randn(256, generator=g).to(dev) * 0.1 for _ in range(2)]
    xd = x.to(dev)
    for epi in (ops.EPI_BF16_RELU, ops.EPI_BF16):
        want = ops.conv3x3(ops.relu(xd[0]), wc[0], bc[0], epi)
        got = ops.conv3x3(xd[0], wc[0], bc[0], epi, relu_input=True)
        assert torch.equal(got, want), epi
    assert not torch.equal(ops.conv3x3(xd[0], wc[0], bc[0], ops.EPI_BF16), want)       # the flag really changes the input
    both = ops.conv3x3_grouped2(xd, wc[0], wc[1], bc[0], bc[1], ops.EPI_BF16_RELU, relu_input=True)
    assert torch.equal(both[0], ops.conv3x3(ops.relu(xd[0]), wc[0], bc[0], ops.EPI_BF16_RELU))
    assert torch.equal(both[1], ops.conv3x3(ops.relu(xd[1]), wc[1], bc[1], ops.EPI_BF16_RELU))


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("bhw_ci_co", [(2, 128, 128, 256, 256), (3, 64, 64, 256, 256), (1, 48, 80, 128, 256), (2, 16, 32, 256, 128)])
def test_direct_convolution_returns_the_bits_of_the_implicit_gemm(dev, dt, bhw_ci_co):
    """m3_conv3x3_direct_grouped2_dt (the DPT residual units at 128 x 128 / 64 x 64 as a direct convolution: LDS halo,
    64-channel slices, output channels split over blockIdx.z) against m3_conv3x3_grouped2_dt on the same operands: BIT-identical for
    every epilogue (plain, ReLU, residual add with one rounding), with and without ReLU on the input, single and 2-group -
    both forms walk K as (channel slice, tap, k-step).  The dispatcher may therefore choose by problem size without
    breaking "a pair gives the same bits alone or in a batch"."""
    b, h, w, ci, co = bhw_ci_co
    from mast3r_slam import _ffi
    splitk = int(_ffi.lib().m3_conv3x3_splitk_bytes(1, h, w, ci, co, 1)) > 0     # (2, 16, 32): a small map the implicit form splits over K
    g = torch.Generator(device="cpu").manual_seed(h + w + ci + co)
    x = torch.randn(2, b, h, w, ci, generator=g).to(dt).to(dev)
    wc = [(torch.randn(co, 3, 3, ci, generator=g) * 0.03).to(dt).to(dev) for _ in range(2)]
    bc = [(torch.randn(co, generator=g) * 0.1).to(dev) for _ in range(2)]
    res = torch.randn(2, b, h, w, co, generator=g).to(dt).to(dev)
    for epi, r in ((ops.EPI_BF16, None), (ops.EPI_BF16_RELU, None), (ops.EPI_BF16_ADD, res)):
        for relu_in in (False, True):
            one = lambda v, direct: ops.conv3x3(x[v], wc[v], bc[v], epi, resid=None if r is None else r[v], relu_input=relu_in, direct=direct)
            d0, i0 = one(0, True), one(0, False)
            both = ops.conv3x3_grouped2(x, wc[0], wc[1], bc[0], bc[1], epi, resid=r, relu_input=relu_in, direct=True)
            assert torch.equal(both[0], d0) and torch.equal(both[1], one(1, True)), (epi, relu_in)
            if splitk:                                           # partial planes summed in another order: close, not equal -
                assert _rel(d0, i0) < 0.5 * TOL16[dt]            # and the dispatcher never sends such a geometry to the direct kernel
                assert not ops.conv3x3_direct_ok(torch.empty(4096, h, w, ci), co)
            else:
                assert torch.equal(d0, i0), (epi, relu_in, _rel(d0, i0))
                assert torch.equal(both[1], one(1, False))
    nb = ops.conv3x3(x[0], wc[0], None, ops.EPI_BF16, direct=True)                           # no bias
    assert splitk or torch.equal(nb, ops.conv3x3(x[0], wc[0], None, ops.EPI_BF16, direct=False))
    xf = torch.relu(x[0].float()).permute(0, 3, 1, 2)
    ref = (F.conv2d(xf, wc[0].float().permute(0, 3, 1, 2), bc[0], padding=1).permute(0, 2, 3, 1) + res[0].float())
    got = ops.conv3x3(x[0], wc[0], bc[0], ops.EPI_BF16_ADD, resid=res[0], relu_input=True, direct=True)
    assert _rel(got, ref) < TOL16[dt]
    assert ops.conv3x3_direct_ok(torch.empty(16, 128, 128, 256), 256) and not ops.conv3x3_direct_ok(torch.empty(1, 128, 128, 256), 256)
    assert not ops.conv3x3_direct_ok(torch.empty(16, 128, 128, 192), 256)


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("cin", [256, 128])
@pytest.mark.parametrize("upsample", [True, False])
@pytest.mark.parametrize("bhw", [(2, 32, 48), (1, 64, 64), (3, 16, 16), (1, 48, 80)])
def test_head0_direct_convolution_with_fused_upsample(dev, dt, cin, upsample, bhw):
    """m3_conv3x3_up_direct_grouped2_dt (DPT head.0 with refinenet1's x2 upsample fused into the LDS halo staging, four 64-channel
    slices, LDS-transposed 16-bit output) against the operators it replaces (k_upsample2x -> implicit-GEMM m3_conv3x3:
    same 16-bit rounding of the upsampled map, fp32 summation order differs) and against a plain torch fp32 chain; the
    2-group launch equals two single launches bit for bit.  Sizes: multiple tiles, a single tile, W = 16 (mod 32)."""
    b, h, w = bhw                                                     # OUTPUT size
    g = torch.Generator(device="cpu").manual_seed(h * 11 + w + cin + int(upsample))
    ih, iw = (h // 2, w // 2) if upsample else (h, w)
    x = torch.randn(2, b, ih, iw, cin, generator=g).to(dt)
    wc = [(torch.randn(128, 3, 3, cin, generator=g) * 0.03).to(dt) for _ in range(2)]
    bc = [torch.randn(128, generator=g) * 0.1 for _ in range(2)]
    d = lambda t: t.to(dev)
    y = ops.conv3x3_up_direct(d(x[0]), d(wc[0]), d(bc[0]), upsample=upsample)
    assert y.shape == (b, h, w, 128) and y.dtype == dt
    xu = ops.upsample2x(d(x[0])) if upsample else d(x[0])
    y_u = ops.conv3x3(xu, d(wc[0]), d(bc[0]), ops.EPI_BF16)
    assert _rel(y, y_u) < 0.5 * TOL16[dt]                             # one 16-bit rounding of sums that differ in their last fp32 bits
    xf = x[0].float().permute(0, 3, 1, 2)
    if upsample:
        xf = F.interpolate(xf, scale_factor=2, mode="bilinear", align_corners=True)
    ref = F.conv2d(xf, wc[0].float().permute(0, 3, 1, 2), bc[0], padding=1).permute(0, 2, 3, 1)
    assert _rel(y, ref) < 2 * TOL16[dt]                               # the interpolated input and the output are rounded once each
    y_nobias = ops.conv3x3_up_direct(d(x[0]), d(wc[0]), None, upsample=upsample)
    assert _rel(y_nobias.float() + d(bc[0]), ref) < 2 * TOL16[dt]
    both = ops.conv3x3_up_direct_grouped2(d(x), d(wc[0]), d(wc[1]), d(bc[0]), d(bc[1]), upsample=upsample)
    assert torch.equal(both[0], y)
    assert torch.equal(both[1], ops.conv3x3_up_direct(d(x[1]), d(wc[1]), d(bc[1]), upsample=upsample))


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("tq_tk_b_h", [(1024, 1024, 16, 16), (256, 256, 2, 3), (672, 672, 2, 4), (200, 150, 2, 3)])
def test_attention_prescaled_deferred_max(dev, dt, tq_tk_b_h):
    """m3_attention_prescaled_dt: q carries scale * log2(e) and the reference maximum enters the S^T MFMA as its
    accumulator initialiser.  fp16 runs the max-tracking loop (reference raised when a tile outgrows it by 2^8), bf16
    the fast loop (reference = first tile's maximum, row sums by MFMA, 2^-64 range keeper, workgroup-wide exact
    recomputation if exp2 overflowed).  Forced branches (guide rule 26): a late key that dominates one query by 2^69
    (rescale / range keeper), a query whose first tile holds its maximum (never rescaled), growth below the deferral
    threshold, and a late key that exceeds the reference by 2^346 (exp2 overflow -> the recomputation path);
    full-tensor float64 reference."""
    tq, tk, b, h = tq_tk_b_h
    g = torch.Generator().manual_seed(tq + h)
    c = h * 64
    q = torch.randn(b, tq, c, generator=g)
    k = torch.randn(b, tk, c, generator=g)
    v = torch.randn(b, tk, c, generator=g)
    q[0, 5, :64] = 6.0 * k[0, tk - 3, :64]                      # query 5 / head 0: one late key dominates (score ~ 6 * 64 * 0.18 >> 8)
    q[0, 7, :64] = 6.0 * k[0, 2, :64]                           # query 7: the dominating key is in the FIRST tile
    q[0, 9, :64] = 0.35 * k[0, min(70, tk - 1), :64]            # query 9: mild growth in a later tile (below the deferral threshold)
    q[1, 11, 64:128] = 30.0 * k[1, tk - 5, 64:128]              # batch 1 / query 11 / head 1: 2^346 above anything before it
    qs = (q * ops.QK_PRESCALE).to(dt)
    kd, vd = k.to(dt), v.to(dt)
    out = torch.full((b, tq, c), 3.0, dtype=dt, device=dev)
    ops.attention(qs.to(dev), kd.to(dev), vd.to(dev), out, nbatch=b, heads=h, tq=tq, tk=tk, q_row_stride=c, kv_row_stride=c,
                  o_row_stride=c, q_batch_stride=tq * c, kv_batch_stride=tk * c, o_batch_stride=tq * c, prescaled=True)
    qf = qs.double().view(b, tq, h, 64).transpose(1, 2)
    kf = kd.double().view(b, tk, h, 64).transpose(1, 2)
    vf = vd.double().view(b, tk, h, 64).transpose(1, 2)
    ref = (torch.softmax(qf @ kf.transpose(-1, -2) * math.log(2.0), -1) @ vf).transpose(1, 2).reshape(b, tq, c)
    tol = 4e-3 if dt == torch.bfloat16 else 6e-4
    assert torch.isfinite(out).all() and _rel(out, ref) < tol
    for row in (5, 7, 9):                                        # the forced rows individually (a whole-tensor norm would hide them)
        assert _rel(out[0, row], ref[0, row]) < 2 * tol, row
    assert _rel(out[1, 11], ref[1, 11]) < 2 * tol
    assert _rel(out[1, 8:16, 64:128], ref[1, 8:16, 64:128]) < 2 * tol     # its neighbours in the recomputed workgroup


@pytest.mark.parametrize("tq_tk_b_h", [(1024, 1024, 4, 16), (672, 672, 2, 4), (200, 150, 2, 3)])
def test_attention_fp16_qk_with_bf16_pv(dev, tq_tk_b_h):
    """M3_DT_F16_PVBF16, the attention form of the fp16 trunk: S = Q K^T on fp16 operands (the logits keep 11 mantissa
    bits), V and the probabilities in bf16 - so the fp16 trunk runs the fast deferred-maximum loop (MODE 2).  Same forced
    branches as the bf16 test (range keeper, first-tile maximum, exp2 overflow -> recomputation); the float64 reference
    takes q, k as the fp16 values and v as the bf16 values the kernel reads.  The logit-side accuracy must be fp16's:
    on rows with one dominating key the result is far closer to the reference than the all-bf16 kernel's."""
    tq, tk, b, h = tq_tk_b_h
    g = torch.Generator().manual_seed(tq + h + 1)
    c = h * 64
    q = torch.randn(b, tq, c, generator=g) * 3.0                 # logits of +-30: the regime where q / k rounding shows
    k = torch.randn(b, tk, c, generator=g)
    v = torch.randn(b, tk, c, generator=g)
    q[0, 5, :64] = 6.0 * k[0, tk - 3, :64]
    q[0, 7, :64] = 6.0 * k[0, 2, :64]
    q[1, 11, 64:128] = 30.0 * k[1, tk - 5, 64:128]
    qs, kd = (q * ops.QK_PRESCALE).half(), k.half()
    vb = v.bfloat16()
    v_as_half = vb.view(torch.float16)                           # bf16 bit patterns inside an fp16 buffer
    out = torch.full((b, tq, c), 3.0, dtype=torch.float16, device=dev)
    ops.attention(qs.to(dev), kd.to(dev), v_as_half.to(dev), out, nbatch=b, heads=h, tq=tq, tk=tk, q_row_stride=c,
                  kv_row_stride=c, o_row_stride=c, q_batch_stride=tq * c, kv_batch_stride=tk * c, o_batch_stride=tq * c,
                  prescaled=True, pv_bf16=True)
    qf = qs.double().view(b, tq, h, 64).transpose(1, 2)
    kf = kd.double().view(b, tk, h, 64).transpose(1, 2)
    vf = vb.double().view(b, tk, h, 64).transpose(1, 2)
    ref = (torch.softmax(qf @ kf.transpose(-1, -2) * math.log(2.0), -1) @ vf).transpose(1, 2).reshape(b, tq, c)
    assert out.dtype == torch.float16 and torch.isfinite(out).all()
    assert _rel(out, ref) < 4e-3                                 # P rounded to bf16: 2^-9 per probability, averaged over the row
    for row in (5, 7):
        assert _rel(out[0, row], ref[0, row]) < 8e-3, row
    assert _rel(out[1, 11], ref[1, 11]) < 8e-3
    # all-bf16 on the SAME inputs: its logits are rounded to 8 bits -> visibly worse against the unrounded float64 result
    full = (torch.softmax((q * ops.QK_PRESCALE).double().view(b, tq, h, 64).transpose(1, 2)
                          @ k.double().view(b, tk, h, 64).transpose(1, 2).transpose(-1, -2) * math.log(2.0), -1)
            @ v.double().view(b, tk, h, 64).transpose(1, 2)).transpose(1, 2).reshape(b, tq, c)
    out_b = torch.empty((b, tq, c), dtype=torch.bfloat16, device=dev)
    ops.attention((q * ops.QK_PRESCALE).bfloat16().to(dev), k.bfloat16().to(dev), vb.to(dev), out_b, nbatch=b, heads=h, tq=tq,
                  tk=tk, q_row_stride=c, kv_row_stride=c, o_row_stride=c, q_batch_stride=tq * c, kv_batch_stride=tk * c,
                  o_batch_stride=tq * c, prescaled=True)
    assert _rel(out, full) < 0.5 * _rel(out_b, full)
    with pytest.raises(TypeError):
        ops.attention(qs.bfloat16().to(dev), kd.bfloat16().to(dev), vb.to(dev), out_b, nbatch=b, heads=h, tq=tq, tk=tk,
                      q_row_stride=c, kv_row_stride=c, o_row_stride=c, q_batch_stride=tq * c, kv_batch_stride=tk * c,
                      o_batch_stride=tq * c, prescaled=True, pv_bf16=True)


@pytest.mark.parametrize("m_n_k", [(256, 192, 64), (2048, 3072, 1024), (16384, 2304, 128)])   # 128 / 256x256 / 256x192 tiles
def test_rope_projection_with_bf16_v_columns(dev, m_n_k):
    """gemm_rope(..., pv_bf16=True) (M3_DT_F16_PVBF16): the q | k columns are the fp16 launch's bits, the v columns
    (>= rope_cols) hold the SAME fp32 results rounded to bf16 instead of fp16 - single and 2-group launches."""
    m, n, k = m_n_k
    g = torch.Generator().manual_seed(n)
    gh, gw = 8, 16
    a = torch.randn(m, k, generator=g).half().to(dev)
    w = (torch.randn(n, k, generator=g) * 0.05).half().to(dev)
    bias = torch.randn(n, generator=g).to(dev)
    gy, gx = torch.meshgrid(torch.arange(gh), torch.arange(gw), indexing="ij")
    pos = torch.stack([gy.reshape(-1), gx.reshape(-1)], -1).to(torch.int32).to(dev)
    rc = (n // 3) * 2 // 64 * 64
    plain = ops.gemm_rope(a, w, bias, pos, rc, q_cols=rc // 2, q_scale=ops.QK_PRESCALE)
    mixed = ops.gemm_rope(a, w, bias, pos, rc, q_cols=rc // 2, q_scale=ops.QK_PRESCALE, pv_bf16=True)
    assert torch.equal(mixed[:, :rc], plain[:, :rc])
    v32 = ops.gemm(a, w, bias, ops.EPI_F32)[:, rc:]
    assert torch.equal(mixed[:, rc:].contiguous().view(torch.bfloat16), v32.bfloat16())
    assert torch.equal(plain[:, rc:], v32.half())
    a2 = torch.stack([a, a.flip(0)])
    both = ops.gemm_grouped2(a2, w, w, bias, bias, ops.EPI_BF16_ROPE, rope=(pos, rc, rc // 2, ops.QK_PRESCALE), pv_bf16=True)
    assert torch.equal(both[0], mixed)
    assert torch.equal(both[1], ops.gemm_rope(a.flip(0).contiguous(), w, bias, pos, rc, q_cols=rc // 2, q_scale=ops.QK_PRESCALE, pv_bf16=True))
    with pytest.raises(TypeError):
        ops.gemm_rope(a.bfloat16(), w.bfloat16(), bias, pos, rc, pv_bf16=True)


def test_attention_fast_path_output_overflow_with_finite_row_sum(dev):
    """bf16 fast loop (MODE 2), round-2 advisor finding: a MID-sequence key ~124 (log2 units) above the first tile's maximum
    with |v| = 32 makes o = sum p v overflow (2^124 * 32 > fp32 max) while l = sum p stays finite; the next tile's range
    keeper would bring l back into range and leave o at inf.  The overflow flag is sticky (l > 2^100 at a range check or
    at the end, or a non-finite o), so the workgroup recomputes the block exactly.  Full float64 reference."""
    tq = tk = 256
    b, h, c = 1, 2, 128
    g = torch.Generator().manual_seed(3)
    q = torch.randn(b, tq, c, generator=g)
    k = torch.randn(b, tk, c, generator=g)
    v = torch.randn(b, tk, c, generator=g)
    key, row = 70, 21                                              # key 70 sits in the second of four key tiles
    v[0, key, :64] = 32.0 * torch.sign(v[0, key, :64])
    kd = k.to(torch.bfloat16)
    excess = 0.0
    for alpha in torch.linspace(8.0, 24.0, 161).tolist():            # pick the multiple of the key that lands the excess in [120, 126]
        q[0, row, :64] = alpha * k[0, key, :64]
        qs = (q * ops.QK_PRESCALE).to(torch.bfloat16)
        sc = qs[0, row, :64].double() @ kd[0, :, :64].double().T
        excess = float(sc[key] - sc[:64].max())
        if 120.0 <= excess <= 126.0:
            break
    assert 120.0 <= excess <= 126.0, excess                          # exp2 stays finite (< 127), p * 32 does not
    vd = v.to(torch.bfloat16)
    out = torch.full((b, tq, c), 3.0, dtype=torch.bfloat16, device=dev)
    ops.attention(qs.to(dev), kd.to(dev), vd.to(dev), out, nbatch=b, heads=h, tq=tq, tk=tk, q_row_stride=c, kv_row_stride=c,
                  o_row_stride=c, q_batch_stride=tq * c, kv_batch_stride=tk * c, o_batch_stride=tq * c, prescaled=True)
    qf = qs.double().view(b, tq, h, 64).transpose(1, 2)
    kf = kd.double().view(b, tk, h, 64).transpose(1, 2)
    vf = vd.double().view(b, tk, h, 64).transpose(1, 2)
    ref = (torch.softmax(qf @ kf.transpose(-1, -2) * math.log(2.0), -1) @ vf).transpose(1, 2).reshape(b, tq, c)
    assert torch.isfinite(out).all()
    assert _rel(out[0, row, :64], ref[0, row, :64]) < 8e-3 and _rel(out, ref) < 4e-3
    assert _rel(out[0, 16:32, :64], ref[0, 16:32, :64]) < 8e-3      # the rest of the recomputed workgroup


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("crop", [(0, 0), (1, 0), (1, 1)])
def test_add_upsample2x_matches_interpolate_crop_add(dev, dt, crop):
    """DPT fusion block glue: bilinear x2 (align_corners) of the coarser path, cropped to the skip connection's size
    (odd token grids), plus the skip connection - fp32 sum, one rounding; against torch fp32."""
    g = torch.Generator().manual_seed(7)
    b, h, w, c = 3, 11, 16, 64
    oh, ow = 2 * h - crop[0], 2 * w - crop[1]
    low = torch.randn(b, h, w, c, generator=g).to(dt)
    y = torch.randn(b, oh, ow, c, generator=g).to(dt)
    out = ops.add_upsample2x(low.to(dev), y.to(dev))
    up = F.interpolate(low.float().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True)
    ref = up[:, :, :oh, :ow].permute(0, 2, 3, 1) + y.float()
    assert out.shape == y.shape and out.dtype == dt
    assert _rel(out, ref) < TOL16[dt]
    # equals the two separate launches up to the one rounding it saves
    sep = ops.add(ops.upsample2x(low.to(dev))[:, :oh, :ow].contiguous(), y.to(dev))
    assert _rel(out, sep) < 2 * TOL16[dt]
    with pytest.raises(ValueError, match="y must be"):
        ops.add_upsample2x(low.to(dev), torch.zeros(b, 2 * h + 1, ow, c, dtype=dt, device=dev))


@pytest.mark.parametrize("dt", DT16)
def test_layernorm_dual2_equals_two_grouped_launches(dev, dt):
    """Decoder block entry: norm1 of a branch's tokens and norm_y of the same tokens as the other branch's memory in
    one pass over the residual stream - bit-identical to the two separate 2-group launches."""
    g = torch.Generator().manual_seed(3)
    m, c = 517, 768
    x = (torch.randn(2, m, c, generator=g) * 3 + 0.5).to(dev)
    prm = [torch.randn(c, generator=g).to(dev) for _ in range(8)]
    own, cross = ((prm[0], prm[1]), (prm[2], prm[3])), ((prm[4], prm[5]), (prm[6], prm[7]))
    y_own, y_cross = ops.layernorm_dual2(x, own, cross, dtype=dt)
    assert torch.equal(y_own, ops.layernorm_grouped2(x, prm[0], prm[1], prm[2], prm[3], dtype=dt))
    assert torch.equal(y_cross, ops.layernorm_grouped2(x, prm[4], prm[5], prm[6], prm[7], swap=True, dtype=dt))


def _fold_problem(m, c, n, seed, dt=torch.float16):
    """A residual stream x [m,c] with outlier channels and a mean offset, a LayerNorm (gamma over a decade, beta) and the
    projection behind it; returns the float64 reference LayerNorm(x) @ W^T + b and the folded operands."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(m, c, generator=g) * 1.5 + 0.3
    x[:, 17] *= 20.0; x[:, c // 2 + 5] -= 12.0                              # massive-activation channels
    gam = torch.exp(torch.randn(c, generator=g) * 0.5); bet = torch.randn(c, generator=g) * 0.1
    W = (torch.randn(n, c, generator=g) * 0.05).to(torch.bfloat16).float(); b = torch.randn(n, generator=g) * 0.1
    ref = F.layer_norm(x.double(), (c,), gam.double(), bet.double(), ops.LN_EPS) @ W.double().T + b.double()
    wf = (W.double() * gam.double()[None]).float().to(dt)
    return x, gam, bet, W, b, ref, wf, wf.double().sum(1).float(), (b.double() + W.double() @ bet.double()).float()


@pytest.mark.parametrize("shape", [(512, 1024, 3072), (2048, 768, 768), (16384, 1024, 1024), (300, 256, 128)])
def test_layernorm_fold_producer_and_consumer(dev, shape):
    """m3_gemm_ex: the residual GEMM also emits the 16-bit copy of the stream and per-row statistics; the projection behind
    the LayerNorm multiplies that RAW copy by gamma-scaled weights and normalises in its epilogue.  Against float64:
    the producer's fp32 stream / copy / statistics exactly as defined, the consumer within the rounding of the raw copy."""
    m, c, n = shape
    x, gam, bet, W, b, ref, wf, cs, fb = _fold_problem(m, c, n, seed=m + c + n)
    g = torch.Generator(device="cpu").manual_seed(5)
    # producer: x' = r + a @ wp^T + bp  (r such that x' is the stream above: a = 0 rows would not exercise the MFMAs)
    kp = 128
    a = torch.randn(m, kp, generator=g).half(); wp = (torch.randn(c, kp, generator=g) * 0.05).half(); bp = torch.randn(c, generator=g)
    r = (x.double() - (a.double() @ wp.double().T + bp.double())).float()
    xs = r.to(dev).clone()
    fo = ops.ln_fold_buffers(m, c, torch.float16, dev)
    out = ops.gemm_ex(a.to(dev), wp.to(dev), bp.to(dev), ops.EPI_F32_ACCUM, out=xs, resid=xs, fold_out=fo)
    plain = ops.gemm(a.to(dev), wp.to(dev), bp.to(dev), ops.EPI_F32_ACCUM, out=r.to(dev).clone(), resid=r.to(dev).clone())
    assert torch.equal(out, plain)                                           # the fp32 stream is what the plain launch writes
    x16, st = fo
    assert torch.equal(x16, out.half())                                      # the copy is the stream rounded once
    slots = st.shape[0]                                                       # 64-column pairs, 128-column halves or one slot per 256- / 192-column tile
    assert slots == ops.ln_slot_count(m, c) and slots in (c // 64, c // 128, c // 192 if c % 192 == 0 else c // 256)
    xo = out.double().cpu().view(m, slots, c // slots)
    assert torch.allclose(st[..., 0].double().cpu().T, xo.sum(-1), rtol=1e-5, atol=1e-3)          # slot-major [slots, m, 2]
    assert torch.allclose(st[..., 1].double().cpu().T, (xo * xo).sum(-1), rtol=1e-5, atol=2e-3)
    # consumer, three epilogues
    ref_d = F.layer_norm(out.double().cpu(), (c,), gam.double(), bet.double(), ops.LN_EPS) @ W.double().T + b.double()
    y = ops.gemm_ex(x16, wf.to(dev), fb.to(dev), ops.EPI_BF16, fold_in=(st, cs.to(dev)))
    shipped = ops.gemm(ops.layernorm(out, gam.to(dev), bet.to(dev), dtype=torch.float16), W.half().to(dev), b.to(dev), ops.EPI_BF16)
    e_fold, e_ship = _rel(y, ref_d), _rel(shipped, ref_d)
    assert e_fold < 1.5e-3 and e_fold < 4 * e_ship + 2e-4, (e_fold, e_ship)   # rounding raw x instead of LN(x): same order of error
    yg = ops.gemm_ex(x16, wf.to(dev), fb.to(dev), ops.EPI_BF16_GELU, fold_in=(st, cs.to(dev)))
    assert _rel(yg, F.gelu(ref_d)) < 2e-3
    if n % 64 == 0:
        t = 16
        pos = torch.stack(torch.meshgrid(torch.arange(4), torch.arange(4), indexing="ij"), -1).reshape(-1, 2).to(torch.int32).to(dev)
        if m % t == 0:
            yr = ops.gemm_ex(x16, wf.to(dev), fb.to(dev), ops.EPI_BF16_ROPE, rope=(pos, n), fold_in=(st, cs.to(dev)))
            plain_r = ops.gemm_rope(ops.layernorm(out, gam.to(dev), bet.to(dev), dtype=torch.float16), W.half().to(dev), b.to(dev), pos, n)
            assert _rel(yr, plain_r) < 3e-3


@pytest.mark.parametrize("c", [768, 1024])
def test_layernorm_fold_is_tile_shape_invariant(dev, c):
    """A row's statistics are ONE expression tree (32-column leaves -> pairs -> halves -> 256- / 192-column top nodes -> total)
    whichever kernel produces or consumes the pieces, so the stream, its copy AND the consumer's output are bitwise the same
    whichever tile shape a launch is dispatched to (64 / 128 / 192 / 256), each of which stores a different level of the tree."""
    m, n = 4096, 1536
    x, gam, bet, W, b, ref, wf, cs, fb = _fold_problem(m, c, n, seed=3)
    g = torch.Generator(device="cpu").manual_seed(9)
    a = torch.randn(m, 256, generator=g).half().to(dev); wp = (torch.randn(c, 256, generator=g) * 0.05).half().to(dev)
    got, shapes = [], set()
    prev = ops._ffi.lib().m3_gemm_set_tile(0)
    try:
        for tile in (64, 128, 192, 256):
            ops._ffi.lib().m3_gemm_set_tile(tile)
            xs = x.to(dev).clone()
            fo = ops.ln_fold_buffers(m, c, torch.float16, dev)
            ops.gemm_ex(a, wp, None, ops.EPI_F32_ACCUM, out=xs, resid=xs, fold_out=fo)
            y = ops.gemm_ex(fo[0], wf.to(dev), fb.to(dev), ops.EPI_BF16_GELU, fold_in=(fo[1], cs.to(dev)))
            got.append((xs, fo[0], y))
            shapes.add(fo[1].shape[0])
    finally:
        ops._ffi.lib().m3_gemm_set_tile(prev)
    assert shapes == ({12, 4} if c == 768 else {16, 8, 4})                    # pairs / halves / top nodes, by what the tile width allows
    for other in got[1:]:
        for p, q in zip(got[0], other):
            assert torch.equal(p, q)


def test_layernorm_fold_two_groups_and_swapped_memory(dev):
    """Two-group launches (the decoder branches): group g's producer fills its half of the copy / statistics; with a_swap the
    consumer of group g multiplies the OTHER stream's copy with the other stream's statistics (cross-attention memory)."""
    m, c, n = 1024, 768, 1536
    P0, P1 = _fold_problem(m, c, n, seed=21), _fold_problem(m, c, n, seed=22)
    x = torch.stack([P0[0], P1[0]]).to(dev)
    g = torch.Generator(device="cpu").manual_seed(2)
    a = torch.randn(2, m, 64, generator=g).half().to(dev); wp = [(torch.randn(c, 64, generator=g) * 0.05).half().to(dev) for _ in range(2)]
    xs = x.clone()
    fo = ops.ln_fold_buffers(m, c, torch.float16, dev, groups=2)
    ops.gemm_ex(a, wp[0], None, ops.EPI_F32_ACCUM, out=xs, resid=xs, w1=wp[1], fold_out=fo)
    for gi in range(2):                                                       # each group = the single-group launch on its half
        x1 = x[gi].clone(); f1 = ops.ln_fold_buffers(m, c, torch.float16, dev)
        ops.gemm_ex(a[gi].contiguous(), wp[gi], None, ops.EPI_F32_ACCUM, out=x1, resid=x1, fold_out=f1)
        assert torch.equal(xs[gi], x1) and torch.equal(fo[0][gi], f1[0])
        assert fo[1][gi].shape != f1[1].shape or torch.equal(fo[1][gi], f1[1])      # (the two launches may store different tree levels)
    wf = [P0[6].to(dev), P1[6].to(dev)]; cs = [P0[7].to(dev), P1[7].to(dev)]; fb = [P0[8].to(dev), P1[8].to(dev)]
    for swap in (False, True):
        y = ops.gemm_ex(fo[0], wf[0], fb[0], ops.EPI_BF16, w1=wf[1], bias1=fb[1], fold_in=(fo[1], cs[0], cs[1]), a_swap=swap)
        for gi in range(2):
            src = 1 - gi if swap else gi
            one = ops.gemm_ex(fo[0][src].contiguous(), wf[gi], fb[gi], ops.EPI_BF16, fold_in=(fo[1][src].contiguous(), cs[gi]))
            assert torch.equal(y[gi], one)


@pytest.mark.parametrize("shape", [(16384, 1024, 256), (2048, 768, 128), (300, 256, 64)])
def test_hi_lo_residual_stream(dev, shape):
    """The hi / lo form of the residual stream (m3_gemm_ex, c_lo): x = hi + lo in two fp16 planes, updated IN PLACE by the
    residual GEMMs together with the rows' statistics.  Against the fp32-stream launches on the same operands: hi is the
    fp32 result rounded to fp16, hi + lo carries it to 2^-21, the statistics are those of the fp32 values; a chain of
    updates stays that close (the stream is re-split after every update, errors do not pile up beyond the roundings)."""
    m, c, k = shape
    g = torch.Generator(device="cpu").manual_seed(m + c)
    mk = lambda: (torch.randn(m, k, generator=g).half().to(dev), (torch.randn(c, k, generator=g) * 0.2).half().to(dev),
                  torch.randn(c, generator=g).to(dev))
    a0, w0, b0 = mk()
    hl = ops.ln_hl_buffers(m, c, dev)
    ops.gemm_ex(a0, w0, b0, ops.EPI_F32, hl=hl)
    x = ops.gemm(a0, w0, b0, ops.EPI_F32)                                     # the fp32-stream twin
    assert torch.equal(hl[0], x.half())
    assert float((ops.hl_to_f32(hl) - x).abs().max()) <= float(x.abs().max()) * 2.0 ** -21
    for step in range(4):
        a, w, b = mk()
        ref = ops.gemm(a, w, b, ops.EPI_F32_ACCUM, out=torch.empty_like(x), resid=ops.hl_to_f32(hl))     # exact twin of this update
        ops.gemm_ex(a, w, b, ops.EPI_F32_ACCUM, hl=hl)
        ops.gemm(a, w, b, ops.EPI_F32_ACCUM, out=x, resid=x)
        assert torch.equal(hl[0], ref.half())                                 # one rounding of (hi + lo) + product
        assert float((ops.hl_to_f32(hl) - ref).abs().max()) <= float(ref.abs().max()) * 2.0 ** -21
        slots = hl[2].shape[0]
        xo = ref.double().cpu().view(m, slots, c // slots)
        assert torch.allclose(hl[2][..., 0].double().cpu().T, xo.sum(-1), rtol=1e-5, atol=1e-3)
        assert torch.allclose(hl[2][..., 1].double().cpu().T, (xo * xo).sum(-1), rtol=1e-5, atol=2e-3)
    assert _rel(ops.hl_to_f32(hl), x) < 1e-6                                  # five updates later: still the fp32 stream


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_layernorm_reads_the_hi_lo_planes(dev, groups, dtype):
    """m3_layernorm_hl_dt (enc_norm / dec_norm on the folded fp16 trunk) == the fp32-input LayerNorm kernel on hi + lo, bit for
    bit, for one group and for the decoder's two groups with their own parameters; against torch within the 16-bit rounding."""
    m, c = 1000, 768
    g = torch.Generator(device="cpu").manual_seed(4 + groups)
    shape = (m, c) if groups == 1 else (2, m, c)
    x = torch.randn(shape, generator=g) * 3.0 + 0.5
    hi = x.half()
    lo = (x - hi.float()).half()
    hl = (hi.to(dev), lo.to(dev))
    par = [(torch.randn(c, generator=g).to(dev), torch.randn(c, generator=g).to(dev)) for _ in range(2)]
    if groups == 1:
        got = ops.layernorm_hl(hl, *par[0], dtype=dtype)
        ref = ops.layernorm(ops.hl_to_f32(hl), *par[0], dtype=dtype)
    else:
        got = ops.layernorm_hl(hl, *par[0], *par[1], dtype=dtype)
        ref = ops.layernorm_grouped2(ops.hl_to_f32(hl), *par[0], *par[1], dtype=dtype)
    assert got.dtype == dtype and torch.equal(got, ref)
    xs = ops.hl_to_f32(hl).double().cpu().reshape(groups, m, c)
    for gi in range(groups):
        t = torch.nn.functional.layer_norm(xs[gi], (c,), par[gi][0].double().cpu(), par[gi][1].double().cpu(), 1e-6)
        assert _rel(got.reshape(groups, m, c)[gi], t) < (3e-3 if dtype == torch.bfloat16 else 4e-4)
