"""Fused attention (ops.attention): every address the key loop forms, on shapes small enough to show a wrong one.

The kernel stages K / V tiles with one per-lane offset per stream and a scalar tile base, reads its fragments through
per-lane offsets whose stage flips every tile, and clamps rows only in the last tile of a Tk that is no multiple of 64.
So the cases are: Tk of one key, exactly one tile, one tile + 1, an odd tile count with a tail, three whole tiles; Tq of one
row, a partial block and two blocks + 1; q | k | v as column slices of ONE [M, 3C] buffer (row stride != width, rows past
Tq / Tk filled with NaN: a read past the end shows) and as separate tensors; kv_batch_shift 0 and 1.  Reference: float64
softmax on the CPU over the operands as the kernel reads them.  The bounds are those tests/test_gpu_model.py applies to
the same kernels (test_attention_vs_softmax_reference, test_attention_prescaled_deferred_max,
test_attention_fp16_qk_with_bf16_pv): 4e-3 where P and O are bf16, 6e-4 where they are fp16, twice that on a single forced
row.  That file keeps them as literals, so they are restated here, not imported.

Each batch item computed alone must equal the batched launch bit for bit (the project's standing invariant).

The small launches (batch 2, heads 3) take the 64-row kernel (QT = 1); the 16 x 16 launches have >= 512 workgroups of 128
rows and take the 128-row kernel (QT = 2), the one the two-view network runs.
"""
import functools
import math

import pytest
import torch

from mast3r_slam import ops

pytestmark = pytest.mark.gpu

GUARD_ROWS = 3
SENTINEL = 7.0
# name -> (16-bit type of q / k / out, prescaled, pv_bf16, bound).  Kernel loop behind it: classic = MODE 0, prescaled fp16 =
# MODE 1 (max tracking), prescaled bf16 and fp16 + pv_bf16 (the fp16 trunk's form) = MODE 2 (deferred maximum)
MODES = {
    "prescaled_fp16_pvbf16": (torch.float16, True, True, 4e-3),
    "prescaled_bf16": (torch.bfloat16, True, False, 4e-3),
    "prescaled_fp16": (torch.float16, True, False, 6e-4),
    "classic_bf16": (torch.bfloat16, False, False, 4e-3),
}
FAST = ["prescaled_fp16_pvbf16", "prescaled_bf16"]            # the MODE 2 launches: range keeper and recomputation exist here
TQS = [1, 63, 129]
TKS = [1, 64, 65, 127, 192]


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm())


@functools.lru_cache(maxsize=None)
def _problem(tq, tk, b, h):
    g = torch.Generator().manual_seed(1000 * tq + tk + b + h)
    c = h * 64
    return (torch.randn(b, tq, c, generator=g), torch.randn(b, tk, c, generator=g), torch.randn(b, tk, c, generator=g))


def _operands(mode, q, k, v):
    """The 16-bit operands as the kernel reads them: (q, k, v as float64 values, q, k, v as stored)."""
    dt, pre, pv, _ = MODES[mode]
    qd = ((q * ops.QK_PRESCALE) if pre else q).to(dt)
    kd = k.to(dt)
    vb = v.bfloat16() if pv else v.to(dt)
    vd = vb.view(torch.float16) if pv else vb                 # pv_bf16: bf16 bit patterns inside the fp16 buffer
    return (qd.double(), kd.double(), vb.double()), (qd, kd, vd)


def _reference(mode, vals, h, shift):
    qf, kf, vf = vals
    b, tq, c = qf.shape
    tk = kf.shape[1]
    qh = qf.view(b, tq, h, 64).transpose(1, 2)
    kh = kf.view(b, tk, h, 64).transpose(1, 2).roll(-shift, 0)            # batch item i attends item (i + shift) % b
    vh = vf.view(b, tk, h, 64).transpose(1, 2).roll(-shift, 0)
    scale = math.log(2.0) if MODES[mode][1] else 0.125
    return (torch.softmax(qh @ kh.transpose(-1, -2) * scale, -1) @ vh).transpose(1, 2).reshape(b, tq, c)


def _views(dev, stored, packed):
    """Device views [b, rows, cols] of q, k, v and their row strides.  packed: column slices of ONE [b, M, 3c] buffer, M =
    max(Tq, Tk), rows past Tq / Tk are NaN."""
    qd, kd, vd = stored
    b, tq, c = qd.shape
    tk = kd.shape[1]
    if not packed:
        return qd.to(dev), kd.to(dev), vd.to(dev), c, c
    m = max(tq, tk)
    buf = torch.full((b, m, 3 * c), float("nan"), dtype=qd.dtype)
    buf[:, :tq, :c] = qd
    buf[:, :tk, c:2 * c] = kd
    buf[:, :tk, 2 * c:] = vd
    buf = buf.to(dev)
    return buf[:, :tq, :c], buf[:, :tk, c:2 * c], buf[:, :tk, 2 * c:], 3 * c, 3 * c


def _attend(dev, mode, qv, kv, vv, h, qrs, krs, shift):
    """One launch over the batch items of the views; returns the padded output [b, tq + GUARD_ROWS, c]."""
    dt, pre, pv, _ = MODES[mode]
    b, tq, tk, c = qv.shape[0], qv.shape[1], kv.shape[1], h * 64
    out = torch.full((b, tq + GUARD_ROWS, c), SENTINEL, dtype=dt, device=dev)
    ops.attention(qv, kv, vv, out, nbatch=b, heads=h, tq=tq, tk=tk, q_row_stride=qrs, kv_row_stride=krs, o_row_stride=c,
                  q_batch_stride=qv.stride(0), kv_batch_stride=kv.stride(0), o_batch_stride=(tq + GUARD_ROWS) * c,
                  kv_batch_shift=shift, prescaled=pre, pv_bf16=pv)
    return out


def _check_launches(dev, mode, q, k, v, h, alone, rows=()):
    """All layouts and shifts of one problem against the float64 reference; `alone`: batch items recomputed one at a time;
    rows: (batch, row, head) triples checked on their own as well.  Returns the failures as text."""
    bound = MODES[mode][3]
    b, tq = q.shape[0], q.shape[1]
    vals, stored = _operands(mode, q, k, v)
    fails = []
    for shift in (0, 1):
        ref = _reference(mode, vals, h, shift)
        for packed in (False, True):
            what = f"{mode} Tq={tq} Tk={k.shape[1]} B={b} H={h} kv_batch_shift={shift} packed={packed}"
            qv, kv, vv, qrs, krs = _views(dev, stored, packed)
            out = _attend(dev, mode, qv, kv, vv, h, qrs, krs, shift)
            err = _rel(out[:, :tq], ref)
            print(f"{what}: rel {err:.3e} (bound {bound:.0e})")
            if not bool(torch.isfinite(out).all()):
                fails.append(f"{what}: non-finite output")
            if not err < bound:
                fails.append(f"{what}: rel {err:.3e} >= {bound:.0e}")
            if not bool((out[:, tq:] == SENTINEL).all()):
                fails.append(f"{what}: guard rows after Tq were written")
            for (bi, row, head) in rows:
                e = _rel(out[bi, row, head * 64:(head + 1) * 64], ref[bi, row, head * 64:(head + 1) * 64])
                print(f"{what}: batch {bi} row {row} head {head}: rel {e:.3e} (bound {2 * bound:.0e})")
                if not e < 2 * bound:
                    fails.append(f"{what}: batch {bi} row {row} head {head}: rel {e:.3e} >= {2 * bound:.0e}")
            for i in alone:
                j = (i + shift) % b
                one = _attend(dev, mode, qv[i:i + 1], kv[j:j + 1], vv[j:j + 1], h, qrs, krs, 0)
                if not torch.equal(one[0], out[i]):
                    fails.append(f"{what}: batch item {i} alone differs from the batched launch")
    return fails


@pytest.mark.parametrize("tk", TKS)
@pytest.mark.parametrize("tq", TQS)
@pytest.mark.parametrize("mode", list(MODES))
def test_small_shapes_every_layout_and_shift(dev, mode, tq, tk):
    b, h = 2, 3
    q, k, v = _problem(tq, tk, b, h)
    fails = _check_launches(dev, mode, q, k, v, h, alone=(0, 1))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("tk", [65, 192])
@pytest.mark.parametrize("mode", FAST)
def test_128_row_kernel_every_layout_and_shift(dev, mode, tk):
    """16 x 16 heads x 2 query blocks = 512 workgroups: the 128-row kernel (QT = 2).  A batch item alone takes the 64-row kernel
    and must still return the same bits."""
    b, h, tq = 16, 16, 129
    q, k, v = _problem(tq, tk, b, h)
    fails = _check_launches(dev, mode, q, k, v, h, alone=(0, 15))
    assert not fails, "\n".join(fails)


def _excess(mode, q, k, bi, row, head, key):
    """log2 units by which `key` exceeds the first tile's maximum for one query, on the operands as the kernel reads them."""
    (qf, kf, _), _ = _operands(mode, q[bi:bi + 1], k[bi:bi + 1], k[bi:bi + 1])
    sc = qf[0, row, head * 64:(head + 1) * 64] @ kf[0, :, head * 64:(head + 1) * 64].T
    return float(sc[key] - sc[:64].max())


@pytest.mark.parametrize("b_h", [(2, 3), (16, 16)], ids=["64_row_kernel", "128_row_kernel"])
@pytest.mark.parametrize("mode", FAST)
def test_scores_growing_after_the_first_tile_trigger_the_range_keeper(dev, mode, b_h):
    """Tk = 192 = three tiles.  Query 5 of batch 0 / head 0 meets a key in the SECOND tile that exceeds the first tile's maximum by
    2^64 .. 2^90: its row sum passes 2^60 (the test in front of the third tile scales o, l by 2^-64 and moves the reference) but
    stays below 2^100 (no recomputation)."""
    b, h = b_h
    tq, tk, key, row = 129, 192, 70, 5
    q, k, v = (t.clone() for t in _problem(tq, tk, b, h))
    excess = 0.0
    for alpha in torch.linspace(4.0, 16.0, 241).tolist():                # the multiple of the key that lands the excess in [64, 90]
        q[0, row, :64] = alpha * k[0, key, :64]
        excess = _excess(mode, q, k, 0, row, 0, key)
        if 64.0 <= excess <= 90.0:
            break
    assert 64.0 <= excess <= 90.0, excess
    fails = _check_launches(dev, mode, q, k, v, h, alone=(0,), rows=[(0, row, 0)])
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("b_h", [(2, 3), (16, 16)], ids=["64_row_kernel", "128_row_kernel"])
@pytest.mark.parametrize("mode", FAST)
def test_exp2_overflow_forces_the_recomputation(dev, mode, b_h):
    """Query 11 of batch 1 / head 1 meets a key in the last tile more than 2^200 above its first tile's maximum: exp2 overflows and
    the workgroup recomputes its block with the max-tracking loop.  Its neighbours in the workgroup are checked with it.
    The item-alone comparison is made where the item alone takes the same kernel (batch 2): the recomputed block is the
    workgroup's, 128 rows in the batched 16 x 16 launch and 64 rows when one of its items runs alone, and the two loops round
    differently, so rows 64..127 of that block legitimately differ in the last bit between the two launches."""
    b, h = b_h
    tq, tk, row = 129, 192, 11
    key = tk - 5
    q, k, v = (t.clone() for t in _problem(tq, tk, b, h))
    q[1, row, 64:128] = 30.0 * k[1, key, 64:128]
    assert _excess(mode, q, k, 1, row, 1, key) > 200.0
    fails = _check_launches(dev, mode, q, k, v, h, alone=(1,) if b == 2 else (), rows=[(1, row, 1), (1, 8, 1), (1, 15, 1)])
    assert not fails, "\n".join(fails)
