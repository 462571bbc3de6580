"""Fused attention (ops.attention) on the routing problem of tests/exact_inputs.py: every query's target key beats every
other key by >= 30 nats (>= 24 for the prescaled entry points, where q is rounded after the scale), so the softmax row is
(1, 0, ...) to below 2^-24 and every output row must EQUAL the target's V row bit for bit.  Each batch item and head has its
own V and its own targets, so a read from the wrong batch item, head, key tile or a key past Tk returns a visibly different
row.  A uniform case (q = 0) pins the row sum and the normalisation, which routing does not.  A third problem (one-hot keys,
integer query tables: every softmax weight an exact power of two) drives known rows through each rescale branch of the
softmax bookkeeping and checks the weighted sum element by element against float64."""
import functools
import math

import pytest
import torch

import exact_inputs as X
from mast3r_slam import ops

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
GUARD_ROWS = 3
# name -> (16-bit type of q / k / out, prescaled, pv_bf16).  Kernel behind it: MODE 0 classic; prescaled bf16 = MODE 2 (fast
# deferred-maximum loop), prescaled fp16 = MODE 1 (max tracking), fp16 + pv_bf16 = MODE 2 with fp16 q / k and bf16 P, V
MODES = {
    "classic_bf16": (torch.bfloat16, False, False),
    "classic_fp16": (torch.float16, False, False),
    "prescaled_bf16": (torch.bfloat16, True, False),
    "prescaled_fp16": (torch.float16, True, False),
    "prescaled_fp16_pvbf16": (torch.float16, True, True),
}
SHAPES = [(1024, 1024, 4, 16), (672, 672, 2, 4), (576, 576, 16, 12), (196, 196, 1, 2), (200, 150, 2, 3), (65, 129, 1, 2), (1, 1, 1, 1)]


def _launch(dev, mode, q, k, v, tq, tk, b, h, shift, packed, scale=0.125, raw_q=False):
    """q, k, v: float32 CPU holders of values exact in the mode's types.  packed: q | k | v (Tq == Tk) or k | v are column slices
    of ONE buffer (row stride 3c / 2c); else three separate tensors.  scale: softmax scale of the classic entry points.
    raw_q: q goes to the prescaled entry points as it is (its scores ARE the exp2 arguments), not times QK_PRESCALE.
    Returns the padded output [b, tq + GUARD_ROWS, c]."""
    dt, pre, pv = MODES[mode]
    c = h * 64
    qd = ((q * ops.QK_PRESCALE) if pre and not raw_q else q).to(dt)
    kd = k.to(dt)
    vd = v.bfloat16().view(torch.float16) if pv else v.to(dt)            # bf16 bit patterns inside the fp16 buffer
    out = torch.full((b, tq + GUARD_ROWS, c), SENTINEL, dtype=dt, device=dev)
    if packed and tq == tk:
        buf = torch.cat([qd, kd, vd], -1).to(dev)                         # [b, t, 3c]
        qv, kv, vv, qrs, krs = buf, buf[..., c:], buf[..., 2 * c:], 3 * c, 3 * c
    elif packed:
        qv = qd.to(dev)
        buf = torch.cat([kd, vd], -1).to(dev)                             # [b, tk, 2c]
        kv, vv, qrs, krs = buf, buf[..., c:], c, 2 * c
    else:
        qv, kv, vv, qrs, krs = qd.to(dev), kd.to(dev), vd.to(dev), c, c
    ops.attention(qv, kv, vv, out, nbatch=b, heads=h, tq=tq, tk=tk, q_row_stride=qrs, kv_row_stride=krs, o_row_stride=c,
                  q_batch_stride=tq * qrs, kv_batch_stride=tk * krs, o_batch_stride=(tq + GUARD_ROWS) * c,
                  kv_batch_shift=shift, scale=scale, prescaled=pre, pv_bf16=pv)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", list(MODES))
def test_routing_attention_returns_the_target_rows_bit_for_bit(dev, mode, shape):
    """Targets in the first key tile, a middle tile and the last (partial) tile incl. the very last key ("spread"), all in the
    first tile ("first": in MODE 2 the fast loop itself answers - no target exceeds the first tile's maximum), and a permutation
    of the keys when Tq == Tk ("perm").  In MODE 2 a target far above the first tile's maximum takes the documented recomputation
    with the MODE 1 loop: wanted coverage.  kv_batch_shift 0 and 1 (B >= 2), q / k / v as column slices of one projection buffer
    and as separate tensors, padded output whose guard rows must stay untouched."""
    tq, tk, b, h = shape
    dt, pre, pv = MODES[mode]
    fails = []
    for placement in X.PLACEMENTS:
        if placement == "perm" and tq != tk:
            continue
        q, k, v, pi = X.routing_problem(tq, tk, b, h, seed=tq + tk + h, placement=placement)
        if pre:                                                            # gap of the operands as the kernel reads them
            gap = X.routing_gap_nats((q * ops.QK_PRESCALE).to(dt).float()[:1], k[:1], pi[:1], math.log(2.0))
            assert gap >= 24.0, gap
        for shift in ((0, 1) if b >= 2 else (0,)):
            exp = X.routing_expected(v, pi, shift).to(dev)
            for packed in (False, True):
                out = _launch(dev, mode, q, k, v, tq, tk, b, h, shift, packed)
                what = f"{mode} Tq={tq} Tk={tk} B={b} H={h} targets={placement} kv_batch_shift={shift} packed={packed} (row = batch * Tq + query, col // 64 = head)"
                try:
                    X.assert_equal_elementwise(out[:, :tq].reshape(b * tq, h * 64), exp.reshape(b * tq, h * 64), what)
                    assert bool((out[:, tq:] == SENTINEL).all()), f"{what}: guard rows after Tq were written"
                except AssertionError as e:
                    fails.append(str(e))
    assert not fails, f"{len(fails)} failing case(s):\n" + "\n".join(fails)


@pytest.mark.parametrize("shape", [(200, 128, 2, 3), (65, 32, 1, 2), (1024, 1024, 2, 4), (7, 2, 2, 1), (5, 1, 1, 1), (130, 256, 2, 2)],
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", list(MODES))
def test_uniform_attention_returns_the_exact_mean(dev, mode, shape):
    """q = 0 and Tk a power of two: every probability is 1 / Tk, the row sum Tk and the integer sum of V are exact in fp32, so
    every output row is the float64 mean of the (shifted) batch item's V rounded ONCE to the output type - the check on the row
    sum, the key-tail mask and the normalisation."""
    tq, tk, b, h = shape
    dt = MODES[mode][0]
    q, k, v = X.uniform_problem(tq, tk, b, h, seed=tk + tq)
    for shift in ((0, 1) if b >= 2 else (0,)):
        out = _launch(dev, mode, q, k, v, tq, tk, b, h, shift, packed=False)
        exp = X.uniform_expected64(v, tq, shift)
        X.assert_equal_elementwise(out[:, :tq].reshape(b * tq, h * 64), exp.reshape(b * tq, h * 64),
                                   f"uniform {mode} Tq={tq} Tk={tk} B={b} H={h} kv_batch_shift={shift}")
        assert bool((out[:, tq:] == SENTINEL).all())


POW2_SHAPES = [(130, 328, 16, 16), (200, 512, 2, 3), (65, 129, 1, 2), (96, 1024, 1, 2), (7, 64, 2, 1)]


@functools.lru_cache(maxsize=len(X.POW2_VARIANTS))
def _pow2_case(dev, shape, variant):
    """One power-of-two problem and its float64 reference per kv_batch_shift (on the device, one batch item at a time), shared
    by the five modes: the shape is the slowest parameter of the test below, so three entries are all that is ever alive."""
    tq, tk, b, h = shape
    q, k, v, info = X.pow2_problem(tq, tk, b, h, seed=tq + tk + h, variant=variant)
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    refs = {}
    for shift in ((0, 1) if b >= 2 else (0,)):
        parts = []
        for i in range(b):
            j = (i + shift) % b
            parts.append(X.pow2_reference(qd[i:i + 1], kd[j:j + 1], vd[j:j + 1], classic=True))
        refs[shift] = {key: torch.cat([p[key] for p in parts]).reshape(b * tq, h * 64) for key in parts[0]}
        assert bool(refs[shift]["gap_ok"].all()), "a log2-weight inside (-30, -12)"
    prof = info["prof"].transpose(1, 2).reshape(b * tq, h).to(dev)                      # [row = batch * Tq + query, head]
    return q, k, v, prof, refs


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", POW2_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_power_of_two_softmax_every_rescale_path(dev, mode, shape):
    """One-hot keys and integer query tables (exact_inputs.pow2_problem): every score is one exact product and every softmax
    weight 2^(s - m) a power of two under any reference m, so the running maximum, every alpha, the deferred update of MODE 1,
    the range keeper of MODE 2 and its overflow recomputation multiply by exact factors, and each row profile sends known rows
    through one of them.  Prescaled entry points get q as it is, classic ones run at scale = ln 2.  Every output element is
    compared with the float64 weighted sum under pow2_bound (c = 8 units of 2^-24 A on the narrow rows, whose sums are exact;
    Tk + 8 elsewhere; E_cls for the classic exponent).  Shapes: 128-row workgroups with a partial query block and a key tail
    of 8; 64-row workgroups with 8 full tiles; a tail of ONE key; 16 tiles; a single tile.  mixed / banded / overflow row
    assignments, kv_batch_shift 0 and 1 (B >= 2), k | v packed and separate, guard rows after Tq.  The largest |diff| / bound
    per mode is printed, not asserted (DESIGN.md records it: up to 0.994, all of it the output rounding - the share of t
    spent beyond u (|ref| + t) was 0.000 on narrow rows and <= 0.001 elsewhere on MI355X)."""
    tq, tk, b, h = shape
    dt, pre, pv = MODES[mode]
    fails, worst, same, total = [], {"narrow": 0.0, "other": 0.0, "narrow t": 0.0, "other t": 0.0}, 0, 0
    for variant in X.POW2_VARIANTS:
        q, k, v, prof, refs = _pow2_case(dev, shape, variant)
        for shift, r in refs.items():
            if pre:                                                         # the score is the exp2 argument itself
                r = dict(r, ecls=torch.zeros_like(r["ecls"]))
            ref, nar, bound, t = r["ref"], r["narrow"], X.pow2_bound(r, tk, dt), X.pow2_allowance(r, tk)
            for packed in (False, True):
                out = _launch(dev, mode, q, k, v, tq, tk, b, h, shift, packed, scale=math.log(2.0), raw_q=True)
                got = out[:, :tq].reshape(b * tq, h * 64)
                diff = (got.double() - ref).abs()
                ratio = torch.nan_to_num(diff / bound, nan=float("inf"))
                # what is left of |diff| after the output rounding u (|ref| + t), as a share of t; outputs that ARE round(ref)
                spent = torch.nan_to_num((diff - (bound - t)).clamp(min=0) / t, nan=float("inf"))
                for key, sel in (("narrow", nar), ("other", ~nar)):
                    if bool(sel.any()):
                        worst[key] = max(worst[key], float(ratio[sel].max()))
                        worst[key + " t"] = max(worst[key + " t"], float(spent[sel].max()))
                same += int((got == ref.to(dt)).sum())
                total += got.numel()
                what = (f"{mode} Tq={tq} Tk={tk} B={b} H={h} {variant} kv_batch_shift={shift} packed={packed} "
                        f"(row = batch * Tq + query, col // 64 = head; mixed: profile (query + head + batch) % {len(X.POW2_PROFILES)})")
                try:
                    X.assert_within(got, ref, bound, what)
                    assert bool((out[:, tq:] == SENTINEL).all()), f"{what}: guard rows after Tq were written"
                except AssertionError as e:
                    hit = prof[(ratio > 1).view(b * tq, h, 64).any(-1)]
                    cnt = torch.bincount(hit, minlength=len(X.POW2_ALL)).tolist()
                    fails.append(f"{e}\n  (row, head) pairs outside their bound, by profile: "
                                 + ", ".join(f"{n} {c}" for n, c in zip(X.POW2_ALL, cnt) if c))
    print(f"pow2 {mode} {'x'.join(map(str, shape))}: worst |diff| / bound narrow {worst['narrow']:.3f} other {worst['other']:.3f}; "
          f"share of t spent beyond the output rounding narrow {worst['narrow t']:.3f} other {worst['other t']:.3f}; "
          f"{same} of {total} outputs are the float64 result rounded once")
    assert not fails, f"{len(fails)} failing case(s):\n" + "\n".join(fails)


def test_constants_match_the_package():
    assert X.QK_PRESCALE == ops.QK_PRESCALE
