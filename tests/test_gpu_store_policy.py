"""Output stores of the row-contiguous epilogues (gemm_common.h: epilogue_rows, serving k_gemm and k_gemm256, dense and
implicit-GEMM convolution) and of the direct convolution (conv_tail.hip).  Their 16-byte stores go out write-through through
a buffer descriptor on the output's base with a 32-bit byte offset per store (the hi / lo planes and the element-wise
fallback through pointers: covered here all the same); what can go wrong there is an offset (the row
pitch, a strided output, the element size), a bound (rows past M, columns past N, the tile's right half outside the map) or a
base (a storage offset, the second group, the output-channel half) - so the shapes are the smallest with an edge in every
one of them, and every output lies inside an allocation whose other rows and columns hold a fixed bit pattern that must still
be there afterwards.

Integer operands (tests/exact_inputs.py): fp32 accumulation is exact, so the kernel must return the float64 result rounded
once to the output type, bit for bit.  GELU and RoPE are checked per element at an exact pre-activation with the bounds
exact_inputs defines for them (their un-rotated v columns bit for bit).

Dense GEMM: M = 274, N = 200, K = 64 in rows of 264 elements (ldc), the output 3 rows into its allocation; one and two groups;
every tile path (64, 128, 256 forced; 192 with N = 192).  Two shapes differ from that because the entry point asks for it:
EPI_BF16_ROPE needs whole 64-column heads (N = 192, ldc = 264), and the LayerNorm-fold producers - the fp32 stream's 16-bit
copy and the hi / lo planes, which are updated in place - take a stream of 256 (192-wide tiles: 768) columns with ldc = N,
so those have guard rows only."""
import contextlib
import functools

import pytest
import torch

import exact_inputs as X
from mast3r_slam import _ffi, ops

pytestmark = pytest.mark.gpu

DT16 = [torch.bfloat16, torch.float16]
M, K, LDC = 274, 64, 264
G0, G1 = 3, 2                                      # guard rows before / after an output
PATTERN = {2: 0x5A5A, 4: 0x5A5A5A5A}               # by element size: a NaN-free, non-zero value no result equals
ITYPE = {2: torch.int16, 4: torch.int32}
TILES = [(64, 200), (128, 200), (256, 200), (192, 192)]      # forced tile, N of the plain epilogues


def _name(dt):
    return str(dt).replace("torch.", "")


@contextlib.contextmanager
def forced_tile(tile):
    L = _ffi.lib()
    prev = L.m3_gemm_set_tile(tile)
    try:
        yield
    finally:
        L.m3_gemm_set_tile(prev)


class Guarded:
    """An output [lead..., rows, ldc] of dtype dt as a view G0 rows into a [G0 + total rows + G1, ldc] allocation filled with
    PATTERN.  check(n): every guard row and, inside the output's rows, every column >= n still holds the pattern."""

    def __init__(self, lead, rows, ldc, dt, dev):
        self.esz = torch.empty((), dtype=dt).element_size()
        self.total = rows * (lead[0] if lead else 1)
        self.big = torch.full((G0 + self.total + G1, ldc), PATTERN[self.esz], dtype=ITYPE[self.esz], device=dev)
        self.view = self.big.view(dt)[G0:G0 + self.total].view(tuple(lead) + (rows, ldc))
        assert self.view.is_contiguous() and self.view.data_ptr() % 16 == 0 and self.view.data_ptr() != self.big.data_ptr()

    def check(self, n, what):
        p = PATTERN[self.esz]
        assert bool((self.big[:G0] == p).all()), f"{what}: rows before the output were written"
        assert bool((self.big[G0 + self.total:] == p).all()), f"{what}: rows behind the output were written"
        assert bool((self.big[G0:G0 + self.total, n:] == p).all()), f"{what}: columns >= N = {n} were written"


def _sq(t, groups):
    return t if groups == 2 else t[0]


def _lead(groups):
    return (2,) if groups == 2 else ()


@functools.lru_cache(maxsize=None)
def _int_problem(n, groups, dev):
    """Integer operands and the float64 product + bias, once per (N, groups)."""
    a, w, b = X.int_gemm(M, n, K, seed=11 * n + groups, groups=groups)
    ref = X.gemm_ref64(a.to(dev), w.to(dev), b.to(dev))
    return a, w, b, ref


@functools.lru_cache(maxsize=None)
def _exact_z_problem(n, groups, dev):
    """gelu_problem per group: operands and the exact float64 pre-activation z [groups, M, n] (on the CPU)."""
    ps = [X.gelu_problem(M, n, seed=50 + 3 * n + g, k=K) for g in range(groups)]
    a, w, b = (torch.stack([p[i] for p in ps]) for i in range(3))
    return a, w, b, X.gemm_ref64(a, w, b)


def _gemm(dev, dt, a, w, b, groups, epi, out, resid=None, **kw):
    ad = _sq(a.to(dt).to(dev), groups).contiguous()
    wd, bd = w.to(dt).to(dev), b.to(dev)
    g1 = dict(w1=wd[1].contiguous(), bias1=bd[1].contiguous()) if groups == 2 else {}
    return ops.gemm_ex(ad, wd[0].contiguous(), bd[0].contiguous(), epi, out=out, resid=resid, **g1, **kw)


# ------------------------------------------------------------------------------------------------------ dense GEMM
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("dt", DT16, ids=_name)
@pytest.mark.parametrize("tile,n", TILES)
def test_dense_strided_guarded_outputs_bit_exact(dev, tile, n, dt, groups):
    """EPI_BF16, EPI_F32, EPI_F32_ACCUM (the fp32 stream updated in place) and EPI_BF16_ADD into guarded, strided outputs."""
    a, w, b, ref = _int_problem(n, groups, dev)
    r16 = X.randint((groups, M, n), -64, 64, seed=n + groups)
    r32 = X.randint((groups, M, n), -4096, 4096, seed=n + groups + 1)
    with forced_tile(tile):
        for epi_name, epi, odt, resid in (("bf16", ops.EPI_BF16, dt, None), ("f32", ops.EPI_F32, torch.float32, None),
                                          ("f32_accum", ops.EPI_F32_ACCUM, torch.float32, r32), ("add", ops.EPI_BF16_ADD, dt, r16)):
            what = f"{epi_name} {_name(dt)} tile={tile} N={n} groups={groups}"
            o = Guarded(_lead(groups), M, LDC, odt, dev)
            rd = None
            if epi == ops.EPI_F32_ACCUM:                      # in place: the stream is the residual
                o.view[..., :n] = _sq(resid, groups).to(dev)
                rd = o.view
            elif resid is not None:
                rd = torch.zeros_like(o.view)
                rd[..., :n] = _sq(resid, groups).to(odt).to(dev)
            got = _gemm(dev, dt, a, w, b, groups, epi, o.view, rd)
            assert got.data_ptr() == o.view.data_ptr()
            exp = ref if resid is None else ref + resid.to(dev).double()
            X.assert_equal_elementwise(got[..., :n].contiguous(), _sq(exp, groups), what)
            o.check(n, what)


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("dt", DT16, ids=_name)
@pytest.mark.parametrize("tile,n", TILES)
def test_dense_gelu_guarded_output(dev, tile, n, dt, groups):
    a, w, b, z = _exact_z_problem(n, groups, dev)
    o = Guarded(_lead(groups), M, LDC, dt, dev)
    with forced_tile(tile):
        got = _gemm(dev, dt, a, w, b, groups, ops.EPI_BF16_GELU, o.view)
    what = f"gelu {_name(dt)} tile={tile} N={n} groups={groups}"
    X.assert_within(got[..., :n].contiguous().cpu(), _sq(X.gelu64(z), groups), _sq(X.gelu_bound(z, dt), groups), what)
    o.check(n, what)


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("dt", DT16, ids=_name)
@pytest.mark.parametrize("tile", [64, 128, 256, 192])
def test_dense_rope_guarded_output(dev, tile, dt, groups):
    """EPI_BF16_ROPE, N = 192 in rows of 264: rotated columns within the RoPE bound, v columns bit for bit - in an fp16 launch
    they are stored as bf16 (pv_bf16)."""
    n, rc, qc, qs = 192, 128, 64, 0.25
    a, w, b, z = _exact_z_problem(n, groups, dev)
    g = torch.Generator().manual_seed(tile)
    pos = torch.stack([torch.randperm(64, generator=g), torch.randperm(64, generator=g)], -1).to(torch.int32)
    e_trig = X.rope_trig_error(64, ops.ROPE_BASE)
    u = torch.finfo(dt).eps / 2
    pv = dt == torch.float16
    o = Guarded(_lead(groups), M, LDC, dt, dev)
    with forced_tile(tile):
        got = _gemm(dev, dt, a, w, b, groups, ops.EPI_BF16_ROPE, o.view, rope=(pos.to(dev).contiguous(), rc, qc, qs), pv_bf16=pv)
    got = got.reshape(groups, M, LDC).cpu()
    for gi in range(groups):
        what = f"rope {_name(dt)} tile={tile} group {gi} of {groups}"
        ref, mag = X.rope_ref64(z[gi], pos.long(), rc, qc, qs, ops.ROPE_BASE)
        X.assert_within(got[gi, :, :rc], ref[:, :rc], u * ref[:, :rc].abs() + mag[:, :rc] * e_trig, what + " rotated columns")
        v = got[gi, :, rc:n].contiguous()
        X.assert_equal_elementwise(v.view(torch.bfloat16) if pv else v, z[gi][:, rc:], what + " v columns")
    o.check(n, f"rope {_name(dt)} tile={tile} groups={groups}")


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("tile", [64, 128, 256, 192])
def test_dense_hi_lo_planes_in_place(dev, tile, groups):
    """EPI_F32 then EPI_F32_ACCUM on hi / lo planes (fp16, updated in place) that lie inside guarded allocations."""
    c = 768 if tile == 192 else 256
    dt = torch.float16
    a, w, _ = X.int_gemm(M, c, K, seed=tile + groups, groups=groups)
    b0, b1 = X.hilo_values((groups, c), seed=3, lim=2.0 ** 14), X.hilo_values((groups, c), seed=4, lim=2.0 ** 13)
    with forced_tile(tile):
        hi, lo = Guarded(_lead(groups), M, c, dt, dev), Guarded(_lead(groups), M, c, dt, dev)
        stats = ops.ln_hl_buffers(M, c, dev, groups)[2]
        hl = (hi.view, lo.view, stats)
        _gemm(dev, dt, a, w, b0, groups, ops.EPI_F32, None, hl=hl)
        ref = X.gemm_ref64(a.to(dev), w.to(dev), b0.to(dev))
        X.assert_equal_elementwise(ops.hl_to_f32(hl), _sq(ref, groups), f"hi/lo EPI_F32 tile={tile} groups={groups}")
        _gemm(dev, dt, a.flip(-2), w, b1, groups, ops.EPI_F32_ACCUM, None, hl=hl)
        ref2 = ref + X.gemm_ref64(a.flip(-2).to(dev), w.to(dev), b1.to(dev))
        assert float(ref2.abs().max()) < 2 ** 15
        what = f"hi/lo EPI_F32_ACCUM tile={tile} groups={groups}"
        X.assert_equal_elementwise(ops.hl_to_f32(hl), _sq(ref2, groups), what)
        X.assert_equal_elementwise(hi.view, _sq(ref2, groups), what + " hi plane")
        hi.check(c, what + " hi plane")
        lo.check(c, what + " lo plane")


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("dt", DT16, ids=_name)
@pytest.mark.parametrize("tile", [64, 128, 256, 192])
def test_dense_fp32_stream_with_16_bit_copy(dev, tile, dt, groups):
    """EPI_F32 / EPI_F32_ACCUM (in place) with the LayerNorm fold's 16-bit copy of the stream: both tensors guarded."""
    c = 768 if tile == 192 else 256
    a, w, b = X.int_gemm(M, c, K, seed=tile + groups + 9, groups=groups)
    ref = X.gemm_ref64(a.to(dev), w.to(dev), b.to(dev))
    with forced_tile(tile):
        o, o16 = Guarded(_lead(groups), M, c, torch.float32, dev), Guarded(_lead(groups), M, c, dt, dev)
        stats = ops.ln_fold_buffers(M, c, dt, dev, groups)[1]
        for step, (epi, resid) in enumerate(((ops.EPI_F32, None), (ops.EPI_F32_ACCUM, o.view))):
            what = f"fp32 stream + copy, step {step} {_name(dt)} tile={tile} groups={groups}"
            _gemm(dev, dt, a, w, b, groups, epi, o.view, resid, fold_out=(o16.view, stats))
            exp = _sq(ref * (step + 1), groups)
            X.assert_equal_elementwise(o.view, exp, what)
            X.assert_equal_elementwise(o16.view, exp, what + " 16-bit copy")
            o.check(c, what)
            o16.check(c, what + " 16-bit copy")


@pytest.mark.parametrize("dt", DT16, ids=_name)
def test_fp32_output_off_the_16_byte_grid_takes_the_elementwise_path(dev, dt):
    """C (and R, in place) 4 bytes off a 16-byte boundary: the element-wise fallback runs, with plain stores, and agrees."""
    n = 200
    a, w, b, ref = _int_problem(n, 1, dev)
    r32 = X.randint((M, n), -4096, 4096, seed=5)
    p = PATTERN[4]
    for tile in (64, 128, 256):
        big = torch.full((1 + (G0 + M + G1) * LDC,), p, dtype=torch.int32, device=dev)
        rows = big[1:].view(G0 + M + G1, LDC)
        view = rows.view(torch.float32)[G0:G0 + M]
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        view[:, :n] = r32.to(dev)
        with forced_tile(tile):
            got = _gemm(dev, dt, a, w, b, 1, ops.EPI_F32_ACCUM, view, view)
        what = f"unaligned f32_accum {_name(dt)} tile={tile}"
        X.assert_equal_elementwise(got[:, :n].contiguous(), ref[0] + r32.to(dev).double(), what)
        assert bool((rows[:G0] == p).all()) and bool((rows[G0 + M:] == p).all()) and bool((rows[G0:G0 + M, n:] == p).all()), what
        assert int(big[0]) == p, what


# ------------------------------------------------------------------------------------- implicit-GEMM convolution
@pytest.mark.parametrize("dt", DT16, ids=_name)
def test_implicit_gemm_conv_guarded_output(dev, dt):
    """1 x 16 x 16 x 64 -> 64, plain and residual add, into a guarded NHWC output."""
    h = wd = 16
    x, wt, bias = X.int_conv(1, h, wd, 64, 64, seed=700)
    ref = X.conv_ref64(x.to(dev), wt.to(dev), bias.to(dev))[0]
    rd = X.randint((1, h, wd, 64), -64, 64, seed=701)
    for epi_name, epi, resid in (("bf16", ops.EPI_BF16, None), ("bf16_add", ops.EPI_BF16_ADD, rd)):
        what = f"implicit conv {epi_name} {_name(dt)}"
        o = Guarded((), h * wd, 64, dt, dev)
        out = o.view.view(1, h, wd, 64)
        got = ops.conv3x3(x[0].to(dt).to(dev), wt[0].to(dt).to(dev), bias[0].to(dev), epi,
                          resid=None if resid is None else resid.to(dt).to(dev), out=out, direct=False)
        assert got.data_ptr() == out.data_ptr()
        X.assert_equal_elementwise(got, ref if resid is None else ref + resid.to(dev).double(), what, hw=(h, wd))
        o.check(64, what)


# ---------------------------------------------------------------------------------------------- direct convolution
def _direct_into(out, x, w0, w1, b0, b1, epi, resid):
    """m3_conv3x3_direct_grouped2_dt as ops.conv3x3(..., direct=True) calls it, into a caller's output."""
    b, h, wd, cin = x.shape[-4:]
    _ffi.call("m3_conv3x3_direct_grouped2_dt", _ffi.ptr(x), _ffi.ptr(w0), _ffi.ptr(w1), _ffi.ptr(b0), _ffi.ptr(b1), _ffi.ptr(out),
              _ffi.ptr(resid), _ffi.ptr(ops.zero_page(x.device)), b, h, wd, cin, w0.shape[0], epi, ops._same16(x, w0, w1),
              _ffi.stream_ptr())


@pytest.mark.parametrize("cout", [128, 256])
@pytest.mark.parametrize("cin", [128, 256])
@pytest.mark.parametrize("wd", [16, 48])
def test_direct_conv_guarded_outputs_bit_exact(dev, wd, cin, cout):
    """B = 1, two groups, H = 16; W = 16 leaves the right half of the 32-pixel tile outside the map.  Plain, ReLU and residual
    add, both 16-bit types, into a guarded [2, 1, H, W, Cout] output."""
    h, groups = 16, 2
    x, wt, bias = X.int_conv(1, h, wd, cin, cout, seed=800 + wd + cin + cout, groups=groups)
    bd = bias.to(dev)
    ref = X.conv_ref64(x.to(dev), wt.to(dev), bd)
    rd = X.randint((groups, 1, h, wd, cout), -64, 64, seed=wd + cin)
    for dt in DT16:
        xd, wdev = x.to(dt).to(dev).contiguous(), wt.to(dt).to(dev).contiguous()
        for epi_name, epi in (("plain", ops.EPI_BF16), ("relu", ops.EPI_BF16_RELU), ("add", ops.EPI_BF16_ADD)):
            what = f"direct conv {epi_name} {_name(dt)} {h}x{wd} {cin}->{cout}"
            o = Guarded((2,), h * wd, cout, dt, dev)
            out = o.view.view(groups, 1, h, wd, cout)
            resid = rd.to(dt).to(dev).contiguous() if epi == ops.EPI_BF16_ADD else None
            _direct_into(out, xd, wdev[0], wdev[1], bd[0].contiguous(), bd[1].contiguous(), epi, resid)
            exp = ref + rd.to(dev).double() if resid is not None else ref
            exp = torch.relu(exp) if epi == ops.EPI_BF16_RELU else exp
            X.assert_equal_elementwise(out, exp, what, hw=(h, wd))
            o.check(cout, what)
