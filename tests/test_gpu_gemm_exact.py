"""Dense GEMM family (m3_gemm_ex through ops.gemm / ops.gemm_grouped2 / ops.gemm_ex) on inputs whose correct answer is EXACT
(tests/exact_inputs.py): integer operands make every partial sum an integer below 2^24, so fp32 accumulation is exact in any
order and the kernel must return the float64 result rounded once to the output type, bit for bit - every tile kernel, both
16-bit types, every linear epilogue, with an edge in every position.  The non-linear epilogues are pinned per element
against float64 evaluated at the exact pre-activation.  The float64 references of the GEMMs are torch.float64 matmuls on the
device (no code shared with the kernels under test); the fold-consumer reference is computed on the CPU."""
import contextlib

import pytest
import torch

import exact_inputs as X
from mast3r_slam import _ffi, ops

pytestmark = pytest.mark.gpu

DT16 = [torch.bfloat16, torch.float16]
TILES = [0, 64, 128, 192, 256]                    # 0 = the dispatcher's own choice
SENTINEL = 7.0                                    # guard rows / columns are pre-filled with it and must keep it


@contextlib.contextmanager
def forced_tile(tile):
    L = _ffi.lib()
    prev = L.m3_gemm_set_tile(tile)
    try:
        yield
    finally:
        L.m3_gemm_set_tile(prev)


def _name(dt):
    return str(dt).replace("torch.", "")


class Failures:
    """Runs every shape of a case and reports all that failed (a loop that stopped at the first would hide the pattern)."""

    def __init__(self):
        self.msgs = []

    @contextlib.contextmanager
    def case(self):
        try:
            yield
        except AssertionError as e:
            self.msgs.append(str(e))

    def done(self):
        assert not self.msgs, f"{len(self.msgs)} failing case(s):\n" + "\n".join(self.msgs)


# --------------------------------------------------------------------------------------------- linear epilogues
# name -> (epilogue, residual kind, out is resid)
LINEAR = {
    "bf16": (ops.EPI_BF16, None, False),
    "f32": (ops.EPI_F32, None, False),
    "f32_accum": (ops.EPI_F32_ACCUM, "f32", False),
    "f32_accum_inplace": (ops.EPI_F32_ACCUM, "f32", True),
    "bf16_add": (ops.EPI_BF16_ADD, "16", False),
    "bf16_add_inplace": (ops.EPI_BF16_ADD, "16", True),
    "bf16_relu": (ops.EPI_BF16_RELU, None, False),
}
# (M, N, K): exact multiples of every tile; M tails 1, 2, 63, 65, 255, 257, 300; N = 4, 68, 132, 196, 260 (partial N tiles of
# every kernel, N % 8 != 0 takes the element-wise store path) and 768 / 2304 for the 192-wide tiles; K = 64 (one K tile) ... 3072
EDGE_SHAPES = [(256, 256, 64), (512, 768, 128), (128, 128, 1024),
               (1, 4, 64), (2, 68, 64), (63, 132, 128), (65, 196, 64), (255, 260, 64), (257, 132, 64), (300, 132, 3072),
               (300, 260, 1024), (256, 4, 64), (256, 68, 128), (256, 196, 64), (256, 260, 64), (257, 768, 64), (300, 2304, 64),
               (2, 4, 3072)]
PADS = (0, 4, 8)                                   # ldc - N: guard columns (ldc % 4 == 0 is the contract)
GUARD_ROWS = 3


def _linear_case(dev, dt, epi_name, m, n, k, use_bias, pad, seed, groups=1, a_swap=False):
    epi, rkind, inplace = LINEAR[epi_name]
    f32 = epi in (ops.EPI_F32, ops.EPI_F32_ACCUM)
    odt = torch.float32 if f32 else dt
    a, w, b = X.int_gemm(m, n, k, seed, groups)
    ad, wd, bd = a.to(dt).to(dev), w.to(dt).to(dev), b.to(dev)
    ldc = n + pad
    lead = (groups,) if groups == 2 else ()
    rows = m + (GUARD_ROWS if groups == 1 else 0)
    big = torch.full(lead + (rows, ldc), SENTINEL, dtype=odt, device=dev)
    out = big[..., :m, :] if groups == 2 else big[:m]
    resid = rd = None
    if rkind is not None:
        r = X.randint(lead + (m, n), -(2 ** 20) + 1, 2 ** 20 - 1, seed + 1) if rkind == "f32" else X.randint(lead + (m, n), -64, 64, seed + 1)
        rd = r.to(odt).to(dev)
        if inplace:
            out[..., :n] = rd
            resid = out
        else:
            resid = torch.full(lead + (m, ldc), SENTINEL, dtype=odt, device=dev)
            resid[..., :n] = rd
    a_eff = ad.flip(0) if a_swap else ad
    ref = X.gemm_ref64(a_eff, wd, bd if use_bias else None, rd)
    if epi == ops.EPI_BF16_RELU:
        ref = torch.relu(ref)
    assert float(ref.abs().max()) < 2 ** 24
    bias = (lambda g: bd[g] if use_bias else None)
    if groups == 1:
        got = ops.gemm(ad[0], wd[0], bias(0), epi, out=out, resid=resid)
    elif a_swap:
        got = ops.gemm_ex(ad, wd[0], bias(0), epi, out=out, resid=resid, w1=wd[1], bias1=bias(1), a_swap=True)
    else:
        got = ops.gemm_grouped2(ad, wd[0], wd[1], bias(0), bias(1), epi, out=out, resid=resid)
    assert got is out and got.dtype == odt
    what = (f"{epi_name} {_name(dt)} M={m} N={n} K={k} ldc={ldc} bias={use_bias} groups={groups} a_swap={a_swap} "
            f"tile={_ffi.lib().m3_gemm_pick_tile(m, n, groups)}")
    X.assert_equal_elementwise(out[..., :n], ref if groups == 2 else ref[0], what)
    if pad:
        assert bool((big[..., n:] == SENTINEL).all()), f"{what}: guard columns [N, ldc) were written"
    if groups == 1:
        assert bool((big[m:] == SENTINEL).all()), f"{what}: guard rows after M were written"
    if resid is not None and not inplace:
        assert bool((resid[..., n:] == SENTINEL).all()) and torch.equal(resid[..., :n], rd), f"{what}: the residual was modified"


@pytest.mark.parametrize("use_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("epi_name", list(LINEAR))
@pytest.mark.parametrize("dt", DT16, ids=_name)
@pytest.mark.parametrize("tile", TILES)
def test_linear_epilogues_edge_shapes_bit_exact(dev, tile, dt, epi_name, use_bias):
    """Every tile kernel forced in turn (and the dispatcher's own choice): out == float64 reference rounded once, guard columns
    (ldc > N) and guard rows after M untouched, the residual operand unmodified."""
    fails = Failures()
    with forced_tile(tile):
        for i, (m, n, k) in enumerate(EDGE_SHAPES):
            with fails.case():
                _linear_case(dev, dt, epi_name, m, n, k, use_bias, PADS[i % 3], seed=1000 + i)
    fails.done()


@pytest.mark.parametrize("epi_name", ["bf16", "f32_accum_inplace", "bf16_add"])
@pytest.mark.parametrize("dt", DT16, ids=_name)
@pytest.mark.parametrize("shape_tile", [((16384, 768, 128), 0), ((16384, 768, 128), 192), ((16384, 768, 128), 128),
                                        ((2048, 3072, 1024), 0), ((2048, 3072, 1024), 256), ((2048, 3072, 1024), 64)],
                         ids=lambda st: f"{st[0][0]}x{st[0][1]}x{st[0][2]}-tile{st[1]}")
def test_linear_epilogues_full_chip_shapes_bit_exact(dev, shape_tile, dt, epi_name):
    """The two shapes the model launches on the big tiles (256 x 192 and 256 x 256: a full round of the chip), and the same
    problems on a small-tile kernel."""
    (m, n, k), tile = shape_tile
    with forced_tile(tile):
        if tile == 0 and n == 768:
            assert _ffi.lib().m3_gemm_pick_tile(m, n, 1) == 192
        _linear_case(dev, dt, epi_name, m, n, k, True, 0, seed=m + n)


@pytest.mark.parametrize("a_swap", [False, True], ids=["own", "a_swap"])
@pytest.mark.parametrize("epi_name", ["bf16", "f32", "f32_accum_inplace", "bf16_add", "bf16_relu"])
@pytest.mark.parametrize("dt", DT16, ids=_name)
@pytest.mark.parametrize("tile", TILES)
def test_grouped_launches_bit_exact(dev, tile, dt, epi_name, a_swap):
    """groups = 2 with different weights and bias per group; a_swap: group g multiplies the OTHER group's rows."""
    fails = Failures()
    with forced_tile(tile):
        for i, (m, n, k) in enumerate([(300, 132, 64), (256, 768, 128), (1024, 260, 64), (65, 4, 128)]):
            for use_bias in (True, False):
                with fails.case():
                    _linear_case(dev, dt, epi_name, m, n, k, use_bias, PADS[(i + 1) % 3], seed=2000 + i, groups=2, a_swap=a_swap)
    fails.done()


@pytest.mark.parametrize("dt", DT16, ids=_name)
def test_grouped_full_chip_shape_bit_exact(dev, dt):
    for a_swap in (False, True):
        _linear_case(dev, dt, "f32_accum_inplace", 16384, 768, 128, True, 0, seed=77, groups=2, a_swap=a_swap)


# ------------------------------------------------------------------------------------------ LayerNorm fold, producer
def _stream_problem(m, c, k, seed, groups):
    """a [g,m,k] in {-1,0,1}, w [g,c,k] with eight +-1 per row, bias in [-7,7]: a w^T + bias is an integer in [-15, 15]."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-1, 2, (groups, m, k), generator=g).float()
    w = torch.zeros(groups, c, k)
    idx = torch.rand(groups, c, k, generator=g).argsort(-1)[..., :8]
    w.scatter_(-1, idx, (torch.randint(0, 2, (groups, c, 8), generator=g) * 2 - 1).float())
    b = torch.randint(-7, 8, (groups, c), generator=g).float()
    return a, w, b


def _check_stats(st, x_ref64, slots, what):
    X.assert_equal_elementwise(st[..., 0], X.slot_sums64(x_ref64, slots)[..., 0], what + " stats: sum")
    X.assert_equal_elementwise(st[..., 1], X.slot_sums64(x_ref64, slots)[..., 1], what + " stats: sum of squares")


FOLD_LAYOUTS = {768: {12, 4}, 1024: {16, 8, 4}}    # pairs / halves / top nodes of the rows' sum tree


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("dt", DT16, ids=_name)
@pytest.mark.parametrize("c", [768, 1024])
def test_fold_producer_copy_and_statistics_bit_exact(dev, c, dt, groups):
    """fold_out: the fp32 stream is the float64 result, the 16-bit copy is that stream rounded once, and the statistics equal
    the float64 per-slot sums EXACTLY (integer stream in [-15, 15]: sums and sums of squares stay below 2^24), per slot and per
    row - for every slot layout ln_slot_count returns (small M and 16384 by the dispatcher's choice, then every tile forced),
    with EPI_F32 and with EPI_F32_ACCUM in place."""
    fails, seen = Failures(), set()
    for m, tile in [(130, 0), (16384, 0), (514, 64), (514, 128), (514, 192), (514, 256)]:
        with forced_tile(tile):
            slots = ops.ln_slot_count(m, c, groups)
            seen.add(slots)
            a, w, b = _stream_problem(m, c, 64, seed=m + c + groups, groups=groups)
            ad, wd, bd = a.to(dt).to(dev), w.to(dt).to(dev), b.to(dev)
            sq = (lambda t: t if groups == 2 else t[0])
            w1 = dict(w1=wd[1], bias1=bd[1]) if groups == 2 else {}
            what = f"fold producer {_name(dt)} M={m} C={c} groups={groups} tile={tile} slots={slots}"
            with fails.case():                                            # EPI_F32: the stream is the product itself
                fo = ops.ln_fold_buffers(m, c, dt, dev, groups)
                ref = X.gemm_ref64(ad, wd, bd)
                assert float(ref.abs().max()) <= 15
                out = ops.gemm_ex(sq(ad), wd[0], bd[0], ops.EPI_F32, fold_out=fo, **w1)
                X.assert_equal_elementwise(out, sq(ref), what + " f32 stream")
                X.assert_equal_elementwise(fo[0], out.to(dt), what + " f32 16-bit copy")
                _check_stats(fo[1], sq(ref), slots, what + " f32")
            with fails.case():                                            # EPI_F32_ACCUM in place: residual chosen so that the
                x = X.randint((groups, m, c), -15, 15, seed=m + 7).to(dev)        # updated stream is a given integer stream
                xs = sq((x.double() - ref).float()).contiguous()
                fo = ops.ln_fold_buffers(m, c, dt, dev, groups)
                fo[1].fill_(SENTINEL)
                out = ops.gemm_ex(sq(ad), wd[0], bd[0], ops.EPI_F32_ACCUM, out=xs, resid=xs, fold_out=fo, **w1)
                assert out is xs
                X.assert_equal_elementwise(out, sq(x), what + " accum stream")
                X.assert_equal_elementwise(fo[0], sq(x), what + " accum 16-bit copy")
                _check_stats(fo[1], sq(x), slots, what + " accum")
    fails.done()
    assert seen == FOLD_LAYOUTS[c], seen


# ------------------------------------------------------------------------------------------------ hi / lo stream
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("shape", [(16384, 1024, 64), (2048, 768, 128), (300, 256, 64), (2, 1024, 64)], ids=str)
def test_hi_lo_stream_reconstructs_exactly(dev, shape, groups):
    """hl = (hi, lo, stats), fp16: values that are multiples of 1/8 below 2^15 are exactly hi + lo, so after EPI_F32 and after
    an EPI_F32_ACCUM update (r_lo read, both planes rewritten in place) hl_to_f32 must return the float64 result exactly, hi is
    that result rounded once to fp16 and lo the exact remainder.  A second pass with an integer stream in [-15, 15] pins the
    statistics of the hi / lo launches exactly as well."""
    m, c, k = shape
    fails = Failures()
    tiles = TILES if m <= 2048 else [0]
    for tile in tiles:
        with forced_tile(tile):
            what = f"hi/lo M={m} C={c} K={k} groups={groups} tile={tile}"
            a, w, _ = X.int_gemm(m, c, k, seed=m + c + tile, groups=groups)
            sq = (lambda t: t if groups == 2 else t[0])
            b0 = X.hilo_values((groups, c), seed=3, lim=2.0 ** 14)
            b1 = X.hilo_values((groups, c), seed=4, lim=2.0 ** 13)
            ad, wd = a.half().to(dev), w.half().to(dev)
            a2 = ad.flip(-2).contiguous()
            w1 = lambda bb: dict(w1=wd[1], bias1=bb[1]) if groups == 2 else {}
            with fails.case():
                hl = ops.ln_hl_buffers(m, c, dev, groups)
                b0d, b1d = b0.to(dev), b1.to(dev)
                assert ops.gemm_ex(sq(ad), wd[0], b0d[0], ops.EPI_F32, hl=hl, **w1(b0d)) is None
                ref = sq(X.gemm_ref64(ad, wd, b0d))
                assert float(ref.abs().max()) < 2 ** 15
                X.assert_equal_elementwise(ops.hl_to_f32(hl), ref, what + " EPI_F32 hi + lo")
                X.assert_equal_elementwise(hl[0], ref, what + " EPI_F32 hi plane")
                X.assert_equal_elementwise(hl[1], ref - hl[0].double(), what + " EPI_F32 lo plane")
                ops.gemm_ex(sq(a2), wd[0], b1d[0], ops.EPI_F32_ACCUM, hl=hl, **w1(b1d))
                ref2 = ref + sq(X.gemm_ref64(a2, wd, b1d))
                assert float(ref2.abs().max()) < 2 ** 15
                X.assert_equal_elementwise(ops.hl_to_f32(hl), ref2, what + " EPI_F32_ACCUM hi + lo")
                X.assert_equal_elementwise(hl[0], ref2, what + " EPI_F32_ACCUM hi plane")
                X.assert_equal_elementwise(hl[1], ref2 - hl[0].double(), what + " EPI_F32_ACCUM lo plane")
            with fails.case():                                            # integer stream: the statistics are exact too
                sa, sw, sb = _stream_problem(m, c, k, seed=m + 11, groups=groups)
                sad, swd, sbd = sa.half().to(dev), sw.half().to(dev), sb.to(dev)
                hl = ops.ln_hl_buffers(m, c, dev, groups)
                slots = hl[2].shape[-3]
                g1 = dict(w1=swd[1], bias1=sbd[1]) if groups == 2 else {}
                ops.gemm_ex(sq(sad), swd[0], sbd[0], ops.EPI_F32, hl=hl, **g1)
                ref = sq(X.gemm_ref64(sad, swd, sbd))
                X.assert_equal_elementwise(hl[0], ref, what + " small hi plane")
                assert not bool(hl[1].any()), what + ": lo plane of an fp16-exact stream must be zero"
                _check_stats(hl[2], ref, slots, what + " small EPI_F32")
                g0 = dict(w1=swd[1]) if groups == 2 else {}
                ops.gemm_ex(sq(sad.flip(-2).contiguous()), swd[0], None, ops.EPI_F32_ACCUM, hl=hl, **g0)
                ref2 = ref + sq(X.gemm_ref64(sad.flip(-2), swd))
                X.assert_equal_elementwise(hl[0], ref2, what + " small accum hi plane")
                _check_stats(hl[2], ref2, slots, what + " small EPI_F32_ACCUM")
    fails.done()


# ------------------------------------------------------------------------------------------------------ GELU
@pytest.mark.parametrize("dt", DT16, ids=_name)
@pytest.mark.parametrize("tile", TILES)
def test_gelu_epilogue_per_element(dev, tile, dt):
    """EPI_BF16_GELU at an exact pre-activation z (operands in multiples of 1/4, bias in multiples of 2^-10):
    |out - gelu64(z)| <= u |gelu64(z)| + 6e-5 + 4 * 2^-24 |z| per element - one rounding to the output type, the approximation
    error gemm_common.h documents for gelu_erf2, four fp32 roundings around the polynomial - including the region where the
    kernel clamps erf's argument (|z| > 3 sqrt(2))."""
    fails = Failures()
    with forced_tile(tile):
        for i, (m, n) in enumerate([(300, 132), (256, 256), (257, 260), (63, 68), (2048, 768)]):
            with fails.case():
                a, w, b = X.gelu_problem(m, n, seed=40 + i)
                ad, wd, bd = a.to(dt).to(dev), w.to(dt).to(dev), b.to(dev)
                z = X.gemm_ref64(ad, wd, bd)
                assert float(z.min()) < -4.5 and float(z.max()) > 4.5
                out = ops.gemm(ad, wd, bd, ops.EPI_BF16_GELU)
                what = f"gelu {_name(dt)} M={m} N={n} tile={tile}"
                X.assert_within(out, X.gelu64(z), X.gelu_bound(z, dt), what)
    fails.done()


# ------------------------------------------------------------------------------------------------------ RoPE
def _positions(dev, seed):
    """64 tokens whose (y, x) cover every position 0 .. 63 on both axes."""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(64, generator=g), torch.randperm(64, generator=g)], -1).to(torch.int32)


@pytest.mark.parametrize("table", [False, True], ids=["per_element", "lds_table"])
@pytest.mark.parametrize("dt_pv", [(torch.bfloat16, False), (torch.float16, False), (torch.float16, True)],
                         ids=["bfloat16", "float16", "float16_pvbf16"])
@pytest.mark.parametrize("tile", TILES)
def test_rope_epilogue_per_element(dev, tile, dt_pv, table):
    """EPI_BF16_ROPE at exact pre-rotation values.  v columns (>= rope_cols) are not rotated: BIT-EXACT (in bf16 with pv_bf16).
    Rotated columns: |out - ref64| <= u |ref| + (|x| + |y|) q_scale E_trig, where E_trig is measured on the reference side
    only (exact_inputs.rope_trig_error: float32 evaluation of the header's angle formula against float64, times 4 for the
    hardware sin / cos) - never fitted to the kernel.  Positions 0 .. 63 on both axes, per-element and LDS-table path."""
    dt, pv = dt_pv
    e_trig = X.rope_trig_error(64, ops.ROPE_BASE)
    print(f"E_trig = {e_trig:.3e}")
    u = torch.finfo(dt).eps / 2
    fails = Failures()
    with forced_tile(tile):
        for i, (m, n, rc, qc, qs) in enumerate([(320, 192, 128, 64, 0.25), (300, 768, 512, 256, ops.QK_PRESCALE),
                                                (2048, 1536, 1024, 512, ops.QK_PRESCALE), (65, 64, 64, 0, 1.0)]):
            if pv and rc == n:
                continue
            with fails.case():
                pos = _positions(dev, seed=i)
                pd = pos.to(dev).contiguous()
                if table:
                    pd = ops.rope_bound(pd, 64)
                a, w, b = X.gelu_problem(m, n, seed=60 + i)
                ad, wd, bd = a.to(dt).to(dev), w.to(dt).to(dev), b.to(dev)
                z = X.gemm_ref64(ad, wd, bd).cpu()
                ref, mag = X.rope_ref64(z, pos.long(), rc, qc, qs, ops.ROPE_BASE)
                out = ops.gemm_ex(ad, wd, bd, ops.EPI_BF16_ROPE, rope=(pd, rc, qc, qs), pv_bf16=pv).cpu()
                what = f"rope {_name(dt)} pv_bf16={pv} table={table} M={m} N={n} rope_cols={rc} q_cols={qc} tile={tile}"
                X.assert_within(out[:, :rc], ref[:, :rc], u * ref[:, :rc].abs() + mag[:, :rc] * e_trig, what + " rotated columns")
                if rc < n:
                    vcols = out[:, rc:].contiguous()
                    X.assert_equal_elementwise(vcols.view(torch.bfloat16) if pv else vcols, z[:, rc:], what + " v columns")
    fails.done()


# ------------------------------------------------------------------------------------------ LayerNorm fold, consumer
@pytest.mark.parametrize("dt", DT16, ids=_name)
@pytest.mark.parametrize("c", [768, 1024])
@pytest.mark.parametrize("tile", TILES)
def test_fold_consumer_per_element(dev, tile, c, dt):
    """fold_in with an integer stream, gamma in {0.5, 1, 2} and integer weights: the 16-bit operands, the statistics, the
    column sums and hence the accumulator are exact; what remains is the fp32 epilogue rstd * (acc - mean * colsum) + bias.
    Bound per element: u |ref| + 16 * 2^-24 rstd (|acc| + |mean colsum|) + 2^-22 |ref|; the count behind the 16 (11 roundings:
    2 mean, 4 var + eps, 2 rsqrt's ulp, 3 mean * colsum, then subtract and multiply) is derived in
    exact_inputs.fold_consumer_bound, and the same formula in float32 on the CPU stays inside it (test_exact_inputs.py).
    Every statistics level a producer can store (pairs / halves / top nodes), one group and two groups with a_swap."""
    fails = Failures()
    with forced_tile(tile):
        for i, (m, n) in enumerate([(130, 136), (300, 256), (1024, 64)]):
            p = X.fold_consumer_problem(m, c, n, seed=c + i)
            ref, rstd, acc_abs, mcs_abs, kappa = X.fold_consumer_ref64(p, ops.LN_EPS)
            assert float(kappa.max()) <= 2.0
            bound = X.fold_consumer_bound(ref, rstd, acc_abs, mcs_abs, dt)
            xd, wf, cs, fb = p["x"].to(dt).to(dev), p["wf"].to(dt).to(dev), p["colsum"].to(dev), p["bias"].to(dev)
            for slots in sorted(FOLD_LAYOUTS[c]):
                st = X.slot_sums64(p["x"], slots).float().to(dev)
                with fails.case():
                    y = ops.gemm_ex(xd, wf, fb, ops.EPI_BF16, fold_in=(st, cs))
                    X.assert_within(y, ref, bound, f"fold consumer {_name(dt)} M={m} C={c} N={n} slots={slots} tile={tile}")
        # two groups, a_swap: group g normalises and multiplies the OTHER stream
        m, n = 258, 136
        P = [X.fold_consumer_problem(m, c, n, seed=c + 50 + g) for g in range(2)]
        xd = torch.stack([q["x"] for q in P]).to(dt).to(dev)
        slots = min(FOLD_LAYOUTS[c])
        st = torch.stack([X.slot_sums64(q["x"], slots).float() for q in P]).to(dev)
        dv = lambda key, g: P[g][key].to(dev) if key != "wf" else P[g][key].to(dt).to(dev)
        for swap in (False, True):
            with fails.case():
                y = ops.gemm_ex(xd, dv("wf", 0), dv("bias", 0), ops.EPI_BF16, w1=dv("wf", 1), bias1=dv("bias", 1),
                                fold_in=(st, dv("colsum", 0), dv("colsum", 1)), a_swap=swap)
                for g in range(2):
                    q = dict(P[g], x=P[1 - g]["x"]) if swap else P[g]
                    ref, rstd, acc_abs, mcs_abs, _ = X.fold_consumer_ref64(q, ops.LN_EPS)
                    X.assert_within(y[g], ref, X.fold_consumer_bound(ref, rstd, acc_abs, mcs_abs, dt),
                                    f"fold consumer {_name(dt)} C={c} group {g} a_swap={swap} tile={tile}")
    fails.done()


def test_constants_match_the_package():
    assert X.QK_PRESCALE == ops.QK_PRESCALE and ops.ROPE_BASE == 100.0
