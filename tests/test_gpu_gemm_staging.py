"""Operand staging of the 256-row dense GEMM kernel (gemm256.hip, tiles 256 x 256 and 256 x 192 forced in turn): the rows a
workgroup stages are addressed from the tile's first row of A and of W, clamped at M and N, and advanced along K once per
K-tile into one of two LDS stages.  What can go wrong there is a base (a tile at m0 > 0 or n0 > 0, the second group, an
operand that starts in the middle of an allocation), a clamp (rows past M or N staged from somewhere else) or the stage
parity when the K loop ends - so the cases are K = 1, 2, 3 and 5 K-tiles, M and N with one to three tiles and an edge in each
position, one and two groups, and operands that are row ranges of larger buffers whose other rows hold a sentinel.

Integer operands (tests/exact_inputs.py): every partial sum is an integer below 2^24, so the kernel must return the float64
result rounded once to the output type, bit for bit.  The non-linear epilogues are checked per element with the bounds
exact_inputs defines for them.  References are float64 matmuls on the device, computed once per problem and shared by the
data types and epilogues that use it."""
import contextlib
import functools

import pytest
import torch

import exact_inputs as X
from mast3r_slam import _ffi, ops

pytestmark = pytest.mark.gpu

DT16 = [torch.bfloat16, torch.float16]
KS = [64, 128, 192, 320]                          # 1, 2, 3, 5 K-tiles
MS = [1, 255, 257, 300, 513]
TILE_NS = {256: [256, 260, 516], 192: [192, 768]}
SENTINEL = 512.0                                  # exact in both 16-bit types; one staged sentinel row moves a sum by >= 512
GUARD_BEFORE, GUARD_AFTER = 37, 5                 # rows around an operand: the operand starts at row 37 of its allocation


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
    """Runs every shape of a case and reports all that failed."""

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


def guarded(rows: torch.Tensor, dt, dev, lead=()):
    """rows [R, K] (CPU float32) as a view into a [37 + R + 5, K] allocation of dtype dt whose other rows hold SENTINEL;
    lead = (2,): the view is reshaped to [2, R / 2, K] (the two groups of a grouped launch, back to back)."""
    r, k = rows.shape
    big = torch.full((GUARD_BEFORE + r + GUARD_AFTER, k), SENTINEL, dtype=dt, device=dev)
    big[GUARD_BEFORE:GUARD_BEFORE + r] = rows.to(dt).to(dev)
    view = big[GUARD_BEFORE:GUARD_BEFORE + r]
    assert view.is_contiguous() and view.data_ptr() % 16 == 0 and (view.data_ptr() - big.data_ptr()) // (2 * k) % 256 != 0
    return view.view(lead + (r // (lead[0] if lead else 1), k)), big


@functools.lru_cache(maxsize=None)
def _problem(m, n, k, groups, dev):
    """Integer operands, bias and the float64 result a w^T + bias, computed once per problem."""
    a, w, b = X.int_gemm(m, n, k, seed=7 * m + 3 * n + k + groups, groups=groups)
    ref = X.gemm_ref64(a.to(dev), w.to(dev), b.to(dev))
    assert float(ref.abs().max()) < 2 ** 24
    return a, w, b, ref


def _launch(dev, dt, a, w, b, groups, epi):
    """a [g,m,k], w [g,n,k], b [g,n] on the CPU -> the launch's output, operands passed as guarded views."""
    m, k = a.shape[-2:]
    av, abig = guarded(a.reshape(groups * m, k), dt, dev, (2,) if groups == 2 else ())
    wv = [guarded(w[g], dt, dev) for g in range(groups)]
    bd = b.to(dev)
    if groups == 2:
        out = ops.gemm_grouped2(av, wv[0][0], wv[1][0], bd[0], bd[1], epi)
    else:
        out = ops.gemm(av, wv[0][0], bd[0], epi)
    for big, r in [(abig, groups * m)] + [(wb, w.shape[-2]) for _, wb in wv]:
        assert bool((big[:GUARD_BEFORE] == SENTINEL).all()) and bool((big[GUARD_BEFORE + r:] == SENTINEL).all())
    return out


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("dt", DT16, ids=_name)
@pytest.mark.parametrize("tile", [256, 192])
def test_staged_rows_bases_and_clamps_bit_exact(dev, tile, dt, groups):
    """Every (K, M, N) of the module's docstring with the 16-bit and the fp32 epilogue: out == float64 reference rounded once."""
    fails = Failures()
    with forced_tile(tile):
        for k in KS:
            for m in MS:
                for n in TILE_NS[tile]:
                    a, w, b, ref = _problem(m, n, k, groups, dev)
                    for epi_name, epi in (("bf16", ops.EPI_BF16), ("f32", ops.EPI_F32)):
                        with fails.case():
                            out = _launch(dev, dt, a, w, b, groups, epi)
                            assert out.dtype == (torch.float32 if epi == ops.EPI_F32 else dt)
                            X.assert_equal_elementwise(out, ref if groups == 2 else ref[0],
                                                       f"staging {epi_name} {_name(dt)} tile={tile} M={m} N={n} K={k} groups={groups}")
    fails.done()


@pytest.mark.parametrize("dt", DT16, ids=_name)
@pytest.mark.parametrize("tile", [256, 192])
def test_first_tile_alone_equals_the_same_rows_of_the_batch(dev, tile, dt):
    """The first 256 rows computed alone == those rows of the M = 513 launch, on the raw bit patterns (and both exact)."""
    n, k = TILE_NS[tile][-1], 320
    a, w, b, ref = _problem(513, n, k, 1, dev)
    with forced_tile(tile):
        for epi in (ops.EPI_BF16, ops.EPI_F32):
            full = _launch(dev, dt, a, w, b, 1, epi)
            alone = _launch(dev, dt, a[:, :256], w, b, 1, epi)
            it = torch.int32 if epi == ops.EPI_F32 else torch.int16
            assert torch.equal(alone.view(it), full[:256].contiguous().view(it)), f"alone != batch: tile={tile} {_name(dt)} epi={epi}"
            X.assert_equal_elementwise(full, ref[0], f"batch tile={tile} {_name(dt)} epi={epi}")


@pytest.mark.parametrize("dt", DT16, ids=_name)
@pytest.mark.parametrize("tile", [256, 192])
def test_gelu_epilogue_on_guarded_views(dev, tile, dt):
    """EPI_BF16_GELU at an exact pre-activation, bound exact_inputs.gelu_bound; M = 300, three K-tiles."""
    m, n = 300, TILE_NS[tile][-1]
    a, w, b = X.gelu_problem(m, n, seed=tile, k=192)
    z = X.gemm_ref64(a.to(dev), w.to(dev), b.to(dev))
    with forced_tile(tile):
        out = _launch(dev, dt, a[None], w[None], b[None], 1, ops.EPI_BF16_GELU)
    X.assert_within(out, X.gelu64(z), X.gelu_bound(z, dt), f"gelu staging {_name(dt)} tile={tile}")


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("tile", [256, 192])
def test_hi_lo_residual_accumulate_on_guarded_views(dev, tile, groups):
    """EPI_F32 then EPI_F32_ACCUM on a hi / lo stream (fp16): hi + lo is the float64 result exactly after both launches."""
    m, c, k = 300, {256: 256, 192: 768}[tile], 192
    a, w, _ = X.int_gemm(m, c, k, seed=tile + groups, groups=groups)
    b0, b1 = X.hilo_values((groups, c), seed=3, lim=2.0 ** 14), X.hilo_values((groups, c), seed=4, lim=2.0 ** 13)
    dt = torch.float16
    sq = (lambda t: t if groups == 2 else t[0])
    lead = (2,) if groups == 2 else ()
    av, _ = guarded(a.reshape(groups * m, k), dt, dev, lead)
    a2v, _ = guarded(a.flip(-2).reshape(groups * m, k), dt, dev, lead)
    wv = [guarded(w[g], dt, dev)[0] for g in range(groups)]
    b0d, b1d = b0.to(dev), b1.to(dev)
    g1 = (lambda bb: dict(w1=wv[1], bias1=bb[1]) if groups == 2 else {})
    with forced_tile(tile):
        hl = ops.ln_hl_buffers(m, c, dev, groups)
        ops.gemm_ex(av, wv[0], b0d[0], ops.EPI_F32, hl=hl, **g1(b0d))
        ref = sq(X.gemm_ref64(a.to(dev), w.to(dev), b0d))
        X.assert_equal_elementwise(ops.hl_to_f32(hl), ref, f"hi/lo EPI_F32 tile={tile} groups={groups}")
        ops.gemm_ex(a2v, wv[0], b1d[0], ops.EPI_F32_ACCUM, hl=hl, **g1(b1d))
        ref2 = ref + sq(X.gemm_ref64(a.flip(-2).to(dev), w.to(dev), b1d))
        assert float(ref2.abs().max()) < 2 ** 15
        X.assert_equal_elementwise(ops.hl_to_f32(hl), ref2, f"hi/lo EPI_F32_ACCUM tile={tile} groups={groups}")
        X.assert_equal_elementwise(hl[0], ref2, f"hi/lo EPI_F32_ACCUM hi plane tile={tile} groups={groups}")


@pytest.mark.parametrize("dt", DT16, ids=_name)
@pytest.mark.parametrize("tile", [256, 192])
def test_rope_epilogue_on_guarded_views(dev, tile, dt):
    """EPI_BF16_ROPE at exact pre-rotation values: v columns bit-exact, rotated columns within u |ref| + (|x| + |y|) E_trig
    (exact_inputs.rope_trig_error, measured on the reference side)."""
    m, n, rc, qc, qs = (300, 768, 512, 256, ops.QK_PRESCALE) if tile == 192 else (300, 256, 128, 64, 0.25)
    e_trig = X.rope_trig_error(64, ops.ROPE_BASE)
    u = torch.finfo(dt).eps / 2
    g = torch.Generator().manual_seed(tile)
    pos = torch.stack([torch.randperm(64, generator=g), torch.randperm(64, generator=g)], -1).to(torch.int32)
    a, w, b = X.gelu_problem(m, n, seed=tile + 1, k=128)
    z = X.gemm_ref64(a, w, b)
    ref, mag = X.rope_ref64(z, pos.long(), rc, qc, qs, ops.ROPE_BASE)
    av, wv = guarded(a, dt, dev)[0], guarded(w, dt, dev)[0]
    with forced_tile(tile):
        out = ops.gemm_ex(av, wv, b.to(dev), ops.EPI_BF16_ROPE, rope=(pos.to(dev).contiguous(), rc, qc, qs)).cpu()
    what = f"rope staging {_name(dt)} tile={tile}"
    X.assert_within(out[:, :rc], ref[:, :rc], u * ref[:, :rc].abs() + mag[:, :rc] * e_trig, what + " rotated columns")
    X.assert_equal_elementwise(out[:, rc:].contiguous(), z[:, rc:], what + " v columns")
