"""Every convolution kernel path on inputs whose correct answer is EXACT (tests/exact_inputs.py; DESIGN.md, "Exact-input
tests"), checked element for element against a reference that shares no code with the kernels: nine shifted slices of the
zero-padded map fed through a float64 matmul on the device.

1. Integer convolution (x, W in [-3, 3], bias and residual in [-64, 64], cin <= 256): every partial sum is an integer below
   2^24, so the 128-row implicit GEMM, the 256-row ping-pong kernel, split-K planes + k_splitk_finish, the sliced single pass,
   the direct kernel and k_conv_tail must all return the float64 result rounded once, bit for bit.  Tap-identity weights make
   a failure name the tap.
2. The fused head tails at an exact r = (xyz, logit): per-element bound derived in exact_inputs.head4_bounds.
3. The fused x2 upsample: a constant-per-channel map (bit-exact, pins border taps at the UPSAMPLED resolution) and single-tap
   weights over multiples of 1/4 (per-element bound, exact_inputs.upsample2x_ref64: pins the patch origin, the far-edge clamp
   and the tile seams); the same two constructions for k_upsample2x / k_add_upsample2x.

A report names (b, y, x, channel) and y % 16, x % 32 - the position inside a 16 x 32 tile of the direct kernels."""
import pytest
import torch

import exact_inputs as X
from mast3r_slam import _ffi, ops
from test_gpu_gemm_exact import DT16, SENTINEL, Failures, _name, forced_tile

pytestmark = pytest.mark.gpu

GUARD = 4096                                       # sentinel elements after an `out=` buffer; they must keep their value

# name -> (epilogue, residual, out is resid, relu_input)
CONV_EPI = {
    "bf16": (ops.EPI_BF16, False, False, False),
    "bf16_relu": (ops.EPI_BF16_RELU, False, False, False),
    "bf16_add": (ops.EPI_BF16_ADD, True, False, False),
    "bf16_add_inplace": (ops.EPI_BF16_ADD, True, True, False),
    "f32": (ops.EPI_F32, False, False, False),
    "f32_accum": (ops.EPI_F32_ACCUM, True, False, False),
    "f32_accum_inplace": (ops.EPI_F32_ACCUM, True, True, False),
    "bf16+relu_in": (ops.EPI_BF16, False, False, True),
    "bf16_relu+relu_in": (ops.EPI_BF16_RELU, False, False, True),
    "bf16_add+relu_in": (ops.EPI_BF16_ADD, True, False, True),
}
DIRECT_EPI = ["bf16", "bf16_relu", "bf16_add", "bf16+relu_in", "bf16_relu+relu_in", "bf16_add+relu_in"]
SOME_EPI = ["bf16", "f32", "bf16_add_inplace", "bf16_relu+relu_in"]


def _splitk_bytes(b, h, w, cin, cout, stride=1):
    return int(_ffi.lib().m3_conv3x3_splitk_bytes(b, h, w, cin, cout, stride))


def _sq(t, groups):
    return t if groups == 2 else t[0]


def _conv_case(dev, dt, prob, epi_name, what, stride=1, use_bias=True, direct=False, seed=0, ref_dtype=torch.float64):
    """One launch of conv3x3_ex on the CPU problem prob = (x [g,b,h,w,cin], w [g,cout,3,3,cin], bias [g,cout]) against the
    shifted-slice reference on the device; g = 1: the single launch, g = 2: the 2-group launch."""
    x, w, bias = prob
    groups = x.shape[0]
    epi, has_resid, inplace, relu_in = CONV_EPI[epi_name]
    odt = torch.float32 if epi in (ops.EPI_F32, ops.EPI_F32_ACCUM) else dt
    xd, wd, bd = x.to(dt).to(dev), w.to(dt).to(dev), bias.to(dev)
    b, h, wid, cin = x.shape[1:]
    cout = w.shape[1]
    oh, ow = X.conv_out_size(h, wid, stride)
    oshape = (groups, b, oh, ow, cout)
    rd = X.randint(oshape, -64, 64, seed + 17).to(odt).to(dev) if has_resid else None
    ref = X.conv_ref64(xd, wd, bd if use_bias else None, rd, stride, relu_in, dtype=ref_dtype)
    if epi == ops.EPI_BF16_RELU:
        ref = torch.relu(ref)
    assert float(ref.abs().max()) < 2 ** 24
    what = f"{what} {epi_name} {_name(dt)} x={tuple(x.shape)} cout={cout} stride={stride} bias={use_bias} groups={groups} direct={direct}"
    out = buf = resid = None
    if not direct:                                                       # the direct kernel allocates its own output
        n = 1
        for s in oshape:
            n *= s
        buf = torch.full((n + GUARD,), SENTINEL, dtype=odt, device=dev)
        out = _sq(buf[:n].view(oshape), groups)
    if has_resid:
        if inplace:
            out.copy_(_sq(rd, groups))
            resid = out
        else:
            resid = _sq(rd, groups).clone()
    g1 = dict(w1=wd[1], bias1=bd[1] if use_bias else None) if groups == 2 else {}
    got = ops.conv3x3_ex(_sq(xd, groups), wd[0], bd[0] if use_bias else None, epi, stride, resid, out, relu_in, direct, **g1)
    assert got.dtype == odt and (direct or got is out)
    X.assert_equal_elementwise(got, _sq(ref, groups), what, hw=(oh, ow))
    if buf is not None:
        assert bool((buf[-GUARD:] == SENTINEL).all()), f"{what}: elements after the output were written"
    if has_resid and not inplace:
        assert torch.equal(resid, _sq(rd, groups)), f"{what}: the residual was modified"


def _tap_problem(b, h, w, cin, cout, seed, groups=1):
    """int_conv's x and bias with the tap-identity weights (rolled by one output channel in group 1)."""
    x, _, bias = X.int_conv(b, h, w, cin, cout, seed, groups)
    w0 = X.tap_identity_weights(cout, cin)
    return x, torch.stack([w0.roll(g, 0) for g in range(groups)]), bias


def _run_shapes(dev, dt, fails, shapes, epis, what, direct=False, tap_first=True):
    """shapes: (b, h, w, cin, cout, stride).  Every shape runs every epilogue in `epis` as a single and as a 2-group launch,
    bias present and absent alternating (so both occur for each path); the first shape also runs the tap-identity weights."""
    k = 0
    for i, (b, h, w, cin, cout, s) in enumerate(shapes):
        for groups in (1, 2):
            prob = X.int_conv(b, h, w, cin, cout, seed=100 * i + groups + h + w, groups=groups)
            for e in epis:
                with fails.case():
                    _conv_case(dev, dt, prob, e, what, s, use_bias=k % 2 == 0, direct=direct, seed=k)
                k += 1
            if tap_first and i == 0:
                with fails.case():
                    _conv_case(dev, dt, _tap_problem(b, h, w, cin, cout, 7 + i, groups), "bf16", what + " TAP-IDENTITY", s,
                               use_bias=groups == 2, direct=direct)


# ----------------------------------------------------------------------------------- 1. integer convolution
# The ragged shapes the 128-row and 256-row kernels are asked to run.  Cin = 64 is 9 K-tiles, so pick_splits sends every map
# with at most 32 output tiles through split-K with 2 slices (the 128-row kernel writing partial planes, then k_splitk_finish):
# the scratch sizes below say so.  RAGGED_NOSPLIT are ragged maps with more than 32 tiles per image, which reach the kernels'
# own epilogues - under forced_tile(128) the 128-row kernel, under forced_tile(256) the ping-pong kernel.
RAGGED = [(1, 1, 1, 64, 4, 1), (1, 2, 3, 64, 4, 1), (1, 20, 28, 64, 36, 1), (1, 20, 28, 64, 36, 2), (1, 15, 17, 64, 68, 2),
          (2, 16, 16, 64, 128, 1)]
RAGGED_NOSPLIT = [(1, 67, 65, 64, 36, 1), (1, 133, 131, 64, 68, 2), (2, 72, 61, 64, 132, 1)]


def _expected_splits(b, h, w, cin, cout, s):
    """Slices of the split-K rule (pick_splits in gemm.hip): 64 / tiles of one image, at most a quarter of the K tiles, at most
    16; 1 below 8 K-tiles or when that gives fewer than 2."""
    oh, ow = X.conv_out_size(h, w, s)
    tiles = -(-oh * ow // 128) * -(-cout // 128)
    nk = 9 * cin // 64
    return 1 if nk < 8 else max(1, min(64 // tiles, nk // 4, 16))


@pytest.mark.parametrize("dt", DT16, ids=_name)
@pytest.mark.parametrize("tile", [128, 256])
def test_implicit_gemm_ragged_shapes_bit_exact(dev, tile, dt):
    """Odd H and W (the last output row and column read padding on one side only), stride 1 and 2, N = 4 / 36 / 68 / 132,
    1 x 1 and 2 x 3 maps where every tap but the centre is padding; on the small maps through 2-slice split-K (asserted), on
    the maps with more than 32 tiles through the forced kernel itself."""
    fails = Failures()
    for b, h, w, cin, cout, s in RAGGED:
        oh, ow = X.conv_out_size(h, w, s)
        assert _expected_splits(b, h, w, cin, cout, s) == 2 and _splitk_bytes(b, h, w, cin, cout, s) == 2 * b * oh * ow * cout * 4
    for shp in RAGGED_NOSPLIT:
        assert _expected_splits(*shp) == 1 and _splitk_bytes(*shp) == 0
    with forced_tile(tile):
        assert _ffi.lib().m3_gemm_pick_tile(300, 36, 1) == tile
        _run_shapes(dev, dt, fails, RAGGED_NOSPLIT, SOME_EPI, f"implicit tile={tile}")
        _run_shapes(dev, dt, fails, RAGGED, SOME_EPI, f"implicit split-K x2 (tile={tile} forced)")
        for b, h, w, cin, cout, s in RAGGED[:2] + RAGGED_NOSPLIT[1:2]:
            with fails.case():
                _conv_case(dev, dt, _tap_problem(b, h, w, cin, cout, 3), "bf16", f"implicit tile={tile} TAP-IDENTITY", s)
    fails.done()


@pytest.mark.parametrize("dt", DT16, ids=_name)
@pytest.mark.parametrize("path", ["splitk2", "tile128", "tile256"])
def test_every_epilogue_bit_exact(dev, path, dt):
    """EPI_BF16, _RELU, _ADD, EPI_F32, EPI_F32_ACCUM, the residual as a separate tensor and in place (out is resid), the first
    three with relu_input - through k_splitk_finish (20 x 28 map), the 128-row kernel's and the ping-pong kernel's own
    epilogue (67 x 65 map: 35 tiles, no split); single and 2-group launches, with and without bias."""
    shape = (1, 20, 28, 64, 36, 1) if path == "splitk2" else (1, 67, 65, 64, 36, 1)
    assert (_splitk_bytes(*shape) > 0) == (path == "splitk2")
    fails = Failures()
    with forced_tile(256 if path == "tile256" else 128):
        _run_shapes(dev, dt, fails, [shape], list(CONV_EPI), path)
    fails.done()


@pytest.mark.parametrize("dt", DT16, ids=_name)
def test_256_row_kernel_on_the_dispatchers_own_choice(dev, dt):
    """(2, 128, 128, 64 -> 256): no split (512 tiles).  The 2-group launch is the one the dispatcher gives to the ping-pong
    kernel (asserted through m3_gemm_pick_tile, the same cost rule); the single launch runs on the dispatcher's choice and
    under forced_tile(256).  The reference is built in float32 on the device: with these integers every partial sum is below
    2^24, so a float32 matmul is exact too (test_exact_inputs.py compares both), at half the memory."""
    b, h, w, cin, cout = 2, 128, 128, 64, 256
    assert _splitk_bytes(b, h, w, cin, cout) == 0
    assert _ffi.lib().m3_gemm_pick_tile(b * h * w, cout, 2) == 256
    fails = Failures()
    for groups in (2, 1):
        prob = X.int_conv(b, h, w, cin, cout, seed=5 + groups, groups=groups)
        for i, e in enumerate(["bf16", "bf16_add", "f32_accum_inplace"]):
            with fails.case():
                _conv_case(dev, dt, prob, e, "implicit dispatcher", use_bias=i != 1, seed=i, ref_dtype=torch.float32)
    with forced_tile(256):
        with fails.case():
            _conv_case(dev, dt, prob, "bf16_relu+relu_in", "implicit tile=256", ref_dtype=torch.float32)
    fails.done()


def _stride2_split_geometry():
    for shp in [(1, 64, 64, 64, 64, 2), (1, 32, 32, 128, 128, 2), (1, 32, 32, 256, 256, 2), (1, 16, 16, 256, 256, 2)]:
        if _splitk_bytes(*shp) > 0:
            return shp
    raise AssertionError("no stride-2 geometry takes split-K any more")


@pytest.mark.parametrize("dt", DT16, ids=_name)
def test_splitk_planes_and_finishing_kernel_bit_exact(dev, dt):
    """fp32 partial planes summed by k_splitk_finish: 9 slices (16 x 16 x 256 -> 256, one image and three), 4 slices
    (32 x 32), one stride-2 geometry; the scratch sizes are asserted so that a change of the rule cannot move a case to another
    path silently.  Every image against the reference."""
    assert _splitk_bytes(1, 16, 16, 256, 256) == 9 * 256 * 256 * 4
    assert _splitk_bytes(3, 16, 16, 256, 256) == 3 * 9 * 256 * 256 * 4
    assert _splitk_bytes(1, 32, 32, 256, 256) == 4 * 1024 * 256 * 4
    s2 = _stride2_split_geometry()
    oh, ow = X.conv_out_size(s2[1], s2[2], 2)
    assert _splitk_bytes(*s2) == _expected_splits(*s2) * oh * ow * s2[4] * 4
    fails = Failures()
    shapes = [(1, 16, 16, 256, 256, 1), (3, 16, 16, 256, 256, 1), (1, 32, 32, 256, 256, 1), s2]
    for shp in shapes:                                                  # planes, not the sliced pass: fewer tiles than CUs
        oh, ow = X.conv_out_size(shp[1], shp[2], shp[5])
        assert 2 * -(-shp[0] * oh * ow // 128) * (shp[4] // 128) < _ffi.lib().m3_device_cu_count()
    _run_shapes(dev, dt, fails, shapes, ["bf16", "bf16_relu+relu_in", "bf16_add_inplace", "f32", "f32_accum"], "split-K planes")
    fails.done()


@pytest.mark.parametrize("dt", DT16, ids=_name)
def test_sliced_single_pass_bit_exact(dev, dt):
    """x [2, 8, 32, 32, 256] -> 256: a split-K geometry (4 slices) whose 256 output tiles reach the CU count, so one pass walks
    the slices itself.  Every image of both groups against the reference - not against the one-image launch."""
    assert _splitk_bytes(1, 32, 32, 256, 256) == 4 * 1024 * 256 * 4
    assert 2 * (8 * 32 * 32 // 128) * (256 // 128) >= _ffi.lib().m3_device_cu_count()
    prob = X.int_conv(8, 32, 32, 256, 256, seed=31, groups=2)
    fails = Failures()
    for i, e in enumerate(["bf16", "bf16_relu+relu_in", "bf16_add", "bf16_add_inplace"]):
        with fails.case():
            _conv_case(dev, dt, prob, e, "sliced single pass", use_bias=i != 1, seed=i)
    with fails.case():
        _conv_case(dev, dt, _tap_problem(8, 32, 32, 256, 256, 9, 2), "bf16", "sliced single pass TAP-IDENTITY", use_bias=False)
    fails.done()


@pytest.mark.parametrize("dt", DT16, ids=_name)
def test_direct_kernel_bit_exact(dev, dt):
    """m3_conv3x3_direct_grouped2_dt forced with direct=True (LDS halo, 64-channel slices, output channels over blockIdx.z):
    two tile rows, W = 16 (mod 32), a lone 16 x 16 tile, Cin and Cout 128 / 256; its three epilogues with and without
    relu_input - against the reference, not against the implicit form."""
    shapes = [(1, 16, 16, 128, 128, 1), (2, 16, 32, 256, 128, 1), (1, 48, 80, 128, 256, 1), (1, 32, 48, 256, 256, 1)]
    fails = Failures()
    _run_shapes(dev, dt, fails, shapes, DIRECT_EPI, "direct", direct=True)
    fails.done()


def _up_direct(xd, wd, bd, use_bias, upsample, groups):
    if groups == 2:
        return ops.conv3x3_up_direct_grouped2(xd, wd[0], wd[1], bd[0] if use_bias else None, bd[1] if use_bias else None, upsample=upsample)
    return ops.conv3x3_up_direct(xd[0], wd[0], bd[0] if use_bias else None, upsample=upsample)


@pytest.mark.parametrize("dt", DT16, ids=_name)
@pytest.mark.parametrize("cin", [128, 256])
def test_conv_tail_kernel_without_upsample_bit_exact(dev, cin, dt):
    """k_conv_tail through conv3x3_up_direct(upsample=False): 16 x 32 output tiles over an 18 x 34 halo - two tile rows, a
    partial tile column at W = 16 (mod 32), a lone 16 x 16 tile, a batch stride; single and 2-group, with and without bias."""
    fails = Failures()
    k = 0
    for i, (b, h, w) in enumerate([(1, 16, 16), (2, 32, 48), (1, 48, 80), (3, 16, 64)]):
        for groups in (1, 2):
            probs = [X.int_conv(b, h, w, cin, 128, seed=40 + i + groups, groups=groups)]
            if i == 0:
                probs.append(_tap_problem(b, h, w, cin, 128, 11, groups))
            for j, (x, wt, bias) in enumerate(probs):
                with fails.case():
                    use_bias = k % 2 == 0
                    k += 1
                    xd, wd, bd = x.to(dt).to(dev), wt.to(dt).to(dev), bias.to(dev)
                    got = _up_direct(xd, wd, bd, use_bias, False, groups)
                    ref = X.conv_ref64(xd, wd, bd if use_bias else None)
                    X.assert_equal_elementwise(got, _sq(ref, groups), f"k_conv_tail plain {_name(dt)} x={tuple(x.shape)} bias={use_bias} "
                                               f"groups={groups}{' TAP-IDENTITY' if j else ''}", hw=(h, w))
    fails.done()


# ------------------------------------------------------------------------------- 2. fused head tails, exact r
def _check_tail(pts, conf, r64, what, hw):
    e1, e2 = X.exp_f32_errors(r64)
    print(f"{what}: E_expm1 = {e1:.3e} E_exp = {e2:.3e}")
    bp, bc = X.head4_bounds(r64, e1, e2)
    rp, rc = X.head4_expected64(r64)
    X.assert_within(pts.cpu(), rp, bp, what + " pts", hw=hw)
    X.assert_within(conf.cpu().unsqueeze(-1), rc.unsqueeze(-1), bc.unsqueeze(-1), what + " conf", hw=hw)


def _dev16(p, dt, dev):
    return {k: (v.to(dt) if k in ("x", "w", "w4") else v).to(dev) for k, v in p.items()}


@pytest.mark.parametrize("dt", DT16, ids=_name)
def test_head4_tail_of_the_implicit_gemm_per_element(dev, dt):
    """conv3x3_relu_head4 on (1, 50, 120, 64): a ragged M (6000 rows = 46.9 tiles).  r = (xyz, logit) is exact in fp32
    (exact_inputs.head4_problem), including pixels with xyz = 0 (the 1e-8 clamp branch, bound 0: pts must be 0); what remains
    is pts = xyz * (expm1f(d) / fmaxf(d, 1e-8f)) and conf = 1 + expf(c), bounded per element by exact_inputs.head4_bounds."""
    p = X.head4_problem(1, 50, 120, 64, seed=170)
    d = _dev16(p, dt, dev)
    fails = Failures()
    for use_bias in (True, False):
        with fails.case():
            r64 = X.head4_r64(p, use_bias=use_bias)[0]
            assert not use_bias or int((r64[..., :3].abs().sum(-1) == 0).sum()) >= 9
            pts, conf = ops.conv3x3_relu_head4(d["x"][0], d["w"][0], d["bias"][0] if use_bias else None, d["w4"][0], d["b4"][0])
            _check_tail(pts, conf, r64, f"conv3x3_relu_head4 {_name(dt)} bias={use_bias}", (50, 120))
    fails.done()


def _dpt_tail(d, groups, upsample, use_bias=True, x=None):
    x = d["x"] if x is None else x
    bias = (lambda g: d["bias"][g] if use_bias else None)
    if groups == 2:
        return ops.dpt_tail_grouped2(x, d["w"][0], d["w"][1], bias(0), bias(1), d["w4"][0], d["w4"][1], d["b4"][0], d["b4"][1], upsample=upsample)
    return ops.dpt_tail(x[0], d["w"][0], bias(0), d["w4"][0], d["b4"][0], upsample=upsample)


@pytest.mark.parametrize("dt", DT16, ids=_name)
@pytest.mark.parametrize("groups", [1, 2])
def test_dpt_tail_without_upsample_per_element(dev, groups, dt):
    """k_conv_tail's tail epilogue (ReLU, 1x1 projection, pointmap post-processing) at an exact r, single and both heads."""
    fails = Failures()
    for i, (b, h, w) in enumerate([(2, 32, 48), (1, 16, 16), (1, 48, 80)]):
        p = X.head4_problem(b, h, w, 128, seed=h + w, groups=groups)
        d = _dev16(p, dt, dev)
        use_bias = i != groups                                            # absent once for each launch form
        with fails.case():
            r64 = _sq(X.head4_r64(p, use_bias=use_bias), groups)
            pts, conf = _dpt_tail(d, groups, False, use_bias)
            _check_tail(pts, conf, r64, f"dpt_tail {_name(dt)} {(b, h, w)} groups={groups} bias={use_bias}", (h, w))
    fails.done()


# -------------------------------------------------------------------------------------- 3. fused x2 upsample
UP_SIZES = [(2, 32, 48), (1, 16, 16), (1, 48, 80), (1, 64, 64)]        # OUTPUT sizes


@pytest.mark.parametrize("dt", DT16, ids=_name)
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("cin", [128, 256])
def test_up_direct_constant_map_bit_exact(dev, cin, groups, dt):
    """(a) x[b, :, :, c] = v[b, c]: every convex blend returns v (to 2^-22 relative; test_exact_inputs.py evaluates the
    formula), so the upsampled map is exactly v and the output must be the integer convolution of the constant map with zero
    padding at the UPSAMPLED resolution, bit for bit: which taps each border and corner pixel sums (a clamp where a zero
    belongs, or padding applied at the input resolution, changes them), the channel slices, batch and group routing."""
    fails = Failures()
    for i, (b, h, w) in enumerate(UP_SIZES):
        with fails.case():
            v, x = X.const_map(b, h // 2, w // 2, cin, seed=60 + i, groups=groups)
            _, wt, bias = X.int_conv(1, 1, 1, cin, 128, seed=70 + i, groups=groups)
            use_bias = i % 2 == 0
            xd, wd, bd = x.to(dt).to(dev), wt.to(dt).to(dev), bias.to(dev)
            got = _up_direct(xd, wd, bd, use_bias, True, groups)
            up = v.to(dev)[:, :, None, None, :].expand(groups, b, h, w, cin)
            ref = X.conv_ref64(up, wd, bd if use_bias else None)
            X.assert_equal_elementwise(got, _sq(ref, groups), f"up_direct constant {_name(dt)} out={(b, h, w)} cin={cin} groups={groups} "
                                       f"bias={use_bias}", hw=(h, w))
    fails.done()


@pytest.mark.parametrize("dt", DT16, ids=_name)
@pytest.mark.parametrize("groups", [1, 2])
def test_dpt_tail_constant_map_per_element(dev, groups, dt):
    """(a) behind the tail epilogue: the constant map makes r exact at the upsampled resolution; head4_bounds on top."""
    fails = Failures()
    for i, (b, h, w) in enumerate(UP_SIZES):
        with fails.case():
            p = X.head4_problem(1, 4, 4, 128, seed=80 + i, groups=groups)
            v, x = X.const_map(b, h // 2, w // 2, 128, seed=90 + i, groups=groups)
            d = _dev16(p, dt, dev)
            r64 = _sq(X.head4_r64(p, x=v[:, :, None, None, :].expand(groups, b, h, w, 128)), groups)
            pts, conf = _dpt_tail(d, groups, True, x=x.to(dt).to(dev))
            _check_tail(pts, conf, r64, f"dpt_tail constant {_name(dt)} out={(b, h, w)} groups={groups}", (h, w))
    fails.done()


@pytest.mark.parametrize("dt", DT16, ids=_name)
@pytest.mark.parametrize("cin", [128, 256])
def test_up_direct_position_through_the_blend_per_element(dev, cin, dt):
    """(b) x in multiples of 1/4, one tap of weight 1 per output channel: output (y, x, co) is ONE interpolated value rounded
    to 16 bits (the output rounding is then exact), zero where the tap falls outside the upsampled map.  Reference: float64
    interpolation with the exact weights; bound u (|ref| + t) + t with t from exact_inputs.upsample2x_ref64 (fp32 coordinate
    arithmetic times the local slope, a few ulps of the blend) - far below what a neighbouring source pixel changes, so a
    patch origin off by one, a wrong far-edge clamp or a patch too small for its tile shows at the seam where it happens."""
    fails = Failures()
    for i, (b, h, w) in enumerate(UP_SIZES + [(1, 32, 16), (1, 16, 32)]):
        for groups in ((1, 2) if i < 2 else (1 + i % 2,)):
            with fails.case():
                x = X.quarter_values((groups, b, h // 2, w // 2, cin), seed=200 + i)
                w0 = X.tap_identity_weights(128, cin, single_tap=True)
                wt = torch.stack([w0.roll(5 * g, 0) for g in range(groups)])
                got = _up_direct(x.to(dt).to(dev), wt.to(dt).to(dev), None, False, True, groups)
                up, t = X.upsample2x_ref64(x)
                ref = torch.stack([X.single_tap_gather(up[g], 128).roll(5 * g, -1) for g in range(groups)])
                tt = torch.stack([X.single_tap_gather(t[g], 128).roll(5 * g, -1) for g in range(groups)])
                X.assert_within(got.cpu(), _sq(ref, groups), _sq(X.upsample_bound(ref, tt, dt), groups),
                                f"up_direct position {_name(dt)} out={(b, h, w)} cin={cin} groups={groups}", hw=(h, w))
    fails.done()


@pytest.mark.parametrize("dt", DT16, ids=_name)
def test_upsample2x_and_add_upsample2x_exact_inputs(dev, dt):
    """k_upsample2x and k_add_upsample2x (with its crop) share the blend's formula: (a) a constant map must come back as v
    (+ the integer residual, one rounding) bit for bit; (b) multiples of 1/4 within the bound of the fused form."""
    fails = Failures()
    for i, (b, h, w, c, crop) in enumerate([(2, 16, 24, 16, (0, 0)), (3, 11, 16, 64, (1, 1)), (1, 32, 8, 8, (1, 0)), (1, 1, 5, 8, (0, 1))]):
        oh, ow = 2 * h - crop[0], 2 * w - crop[1]
        what = f"{_name(dt)} in={(b, h, w, c)} crop={crop}"
        # |y| >= 8 > |v|: a blend that returns v (1 +- 2^-23) plus y = -v would leave a tiny non-zero sum where 0 is exact
        y = X.randint((b, oh, ow, c), 8, 64, seed=300 + i) * (X.randint((b, oh, ow, c), 0, 1, seed=301 + i) * 2 - 1)
        with fails.case():
            v, x = X.const_map(b, h, w, c, seed=310 + i)
            exp = v[0][:, None, None, :].expand(b, 2 * h, 2 * w, c)
            X.assert_equal_elementwise(ops.upsample2x(x[0].to(dt).to(dev)), exp, "upsample2x constant " + what, hw=(2 * h, 2 * w))
            got = ops.add_upsample2x(x[0].to(dt).to(dev), y.to(dt).to(dev))
            X.assert_equal_elementwise(got, exp[:, :oh, :ow].double() + y.double(), "add_upsample2x constant " + what, hw=(oh, ow))
        with fails.case():
            x = X.quarter_values((b, h, w, c), seed=320 + i)
            ref, t = X.upsample2x_ref64(x)
            X.assert_within(ops.upsample2x(x.to(dt).to(dev)).cpu(), ref, X.upsample_bound(ref, t, dt), "upsample2x position " + what,
                            hw=(2 * h, 2 * w))
            refa = ref[:, :oh, :ow] + y.double()
            ta = t[:, :oh, :ow] + 2.0 ** -23 * refa.abs()               # the fp32 sum blend + y: one rounding (two allowed)
            got = ops.add_upsample2x(x.to(dt).to(dev), y.to(dt).to(dev)).cpu()
            X.assert_within(got, refa, X.upsample_bound(refa, ta, dt), "add_upsample2x position " + what, hw=(oh, ow))
    fails.done()
