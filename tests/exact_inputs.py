"""Inputs for which the correct answer of a kernel is EXACT, and an element-wise checker.

Two constructions ("Exact-input tests"):

* integer GEMM: operands, bias and residual hold small integers (or integers times a power of two), so every product and
  every partial sum is an integer below 2^24: fp32 accumulation is exact in ANY order, on any tile shape.  The kernel must
  return the float64 result rounded once to the output type, bit for bit.
* routing attention: key j carries the code of j's 10 bits in {-1, +1}, query i is 20 x the code of its target pi(i).  The
  target's score beats every other key's by >= 30 nats, so the softmax row is (1, 0, ...) to below 2^-24 and the output row
  must be V[pi(i)] bit for bit.

Plain helper module: CPU tensors only, seeded, no GPU import.  tests/test_exact_inputs.py checks the promises made here
without any kernel.
"""
from __future__ import annotations

import math

import numpy as np
import torch

LOG2E = 1.4426950408889634
QK_PRESCALE = 0.125 * LOG2E                     # what ops.QK_PRESCALE is (asserted equal in the GPU tests)


def _gen(seed: int) -> torch.Generator:
    return torch.Generator(device="cpu").manual_seed(int(seed))


def randint(shape, lo: int, hi: int, seed: int) -> torch.Tensor:
    """float32 tensor of integers in [lo, hi] (both ends included)."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed)).float()


# ------------------------------------------------------------------------------------------------ integer GEMM
def int_gemm(m: int, n: int, k: int, seed: int, groups: int = 1, a_lim: int = 3, w_lim: int = 3, bias_lim: int = 64):
    """A [groups, m, k] in [-a_lim, a_lim], W [groups, n, k] in [-w_lim, w_lim], bias [groups, n] in [-bias_lim, bias_lim];
    float32 holders of integers (all exact in bf16 and fp16).  Different weights / bias per group."""
    g = _gen(seed)
    a = torch.randint(-a_lim, a_lim + 1, (groups, m, k), generator=g).float()
    w = torch.randint(-w_lim, w_lim + 1, (groups, n, k), generator=g).float()
    b = torch.randint(-bias_lim, bias_lim + 1, (groups, n), generator=g).float()
    return a, w, b


def gemm_ref64(a, w, bias=None, resid=None) -> torch.Tensor:
    """float64 a @ w^T (+ bias) (+ resid); leading group dimensions are batched.  Works on any device: on the GPU this is
    torch's float64 matmul, which shares no code with the kernels under test."""
    ref = a.double() @ w.double().transpose(-1, -2)
    if bias is not None:
        ref = ref + bias.double().unsqueeze(-2)
    if resid is not None:
        ref = ref + resid.double()
    return ref


def slot_sums64(x: torch.Tensor, slots: int) -> torch.Tensor:
    """LayerNorm-fold statistics of a stream x [..., m, c] in the producer's layout [..., slots, m, 2]: per row and slot of
    c / slots columns (sum, sum of squares), float64."""
    m, c = x.shape[-2:]
    xs = x.double().reshape(x.shape[:-2] + (m, slots, c // slots))
    st = torch.stack([xs.sum(-1), (xs * xs).sum(-1)], -1)                  # [..., m, slots, 2]
    return st.transpose(-3, -2).contiguous()


def hilo_values(shape, seed: int, lim: float = 2.0 ** 15) -> torch.Tensor:
    """Multiples of 1/8 with |x| < lim (<= 2^15): fp16(x) + fp16(x - fp16(x)) == x exactly."""
    n = int(lim * 8) - 1
    return torch.randint(-n, n + 1, tuple(shape), generator=_gen(seed)).float() / 8.0


# --------------------------------------------------------------------------------- non-linear epilogues: exact z
def gelu_problem(m: int, n: int, seed: int, k: int = 64):
    """A in multiples of 1/4 within [-1/2, 1/2], W in {-1, 0, 1}, bias in multiples of 2^-10 within [-1, 1]: the
    pre-activation z = A W^T + bias is exact in fp32 (a multiple of 2^-10 below 2^6: 16 bits), spread over [-6, 6] and
    beyond with most of its mass in [-3, 3]."""
    g = _gen(seed)
    a = torch.randint(-2, 3, (m, k), generator=g).float() / 4.0
    w = torch.randint(-1, 2, (n, k), generator=g).float()
    b = torch.randint(-1024, 1025, (n,), generator=g).float() / 1024.0
    return a, w, b


def gelu64(z: torch.Tensor) -> torch.Tensor:
    z = z.double()
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def gelu_bound(z64: torch.Tensor, dt) -> torch.Tensor:
    """|out - gelu64(z)| allowed per element: one rounding to the output type, the approximation error the kernel's header
    documents for gelu_erf2 (6e-5), and four fp32 roundings around the polynomial relative to |z|."""
    u = torch.finfo(dt).eps / 2
    return u * gelu64(z64).abs() + 6e-5 + 4 * 2.0 ** -24 * z64.abs()


def rope_trig_error(max_pos: int = 64, base: float = 100.0) -> float:
    """E_trig of the RoPE bound, measured on the REFERENCE side only: the header's formula position * base^(-i/16) evaluated in
    float32 with float32 cos / sin against float64 cos / sin of the float64 angle, maximum over positions < max_pos and the
    16 frequencies, times 4 (margin for the hardware sin / cos, whose accuracy is not documented)."""
    p = np.arange(max_pos, dtype=np.float64)[:, None]
    i = np.arange(16, dtype=np.float64)[None, :]
    ang64 = p * base ** (-i / 16.0)
    f32 = np.power(np.float32(base), (-i / 16.0).astype(np.float32)).astype(np.float32)
    ang32 = (p.astype(np.float32) * f32).astype(np.float32)
    e = max(np.abs(np.cos(ang32).astype(np.float64) - np.cos(ang64)).max(),
            np.abs(np.sin(ang32).astype(np.float64) - np.sin(ang64)).max())
    return 4.0 * float(e)


def rope_ref64(z: torch.Tensor, pos_yx: torch.Tensor, rope_cols: int, q_cols: int = 0, q_scale: float = 1.0, base: float = 100.0):
    """float64 RoPE-2D of the exact pre-rotation values z [m, n] (row r is token r % T, pos_yx int [T, 2] = (y, x)): in every
    64-wide head below rope_cols dims 0..31 rotate with y, 32..63 with x, element i pairs with i + 16, angle pos * base^(-i/16);
    columns < q_cols are then multiplied by float32(q_scale).  Returns (ref, mag): mag = |x| + |y| of the rotated pair
    (times the scale), 0 on the columns that are not rotated."""
    m, n = z.shape
    t = pos_yx.shape[0]
    z = z.double()
    ref, mag = z.clone(), torch.zeros_like(z)
    tok = torch.arange(m) % t
    freq = torch.tensor(base, dtype=torch.float64) ** (-torch.arange(16, dtype=torch.float64) / 16.0)
    qs = float(np.float32(q_scale))
    for blk in range(rope_cols // 32):
        p = pos_yx[tok, blk & 1].double()[:, None]
        c, s = torch.cos(p * freq), torch.sin(p * freq)
        x, y = z[:, blk * 32:blk * 32 + 16], z[:, blk * 32 + 16:blk * 32 + 32]
        sc = qs if blk * 32 < q_cols else 1.0
        ref[:, blk * 32:blk * 32 + 16] = (x * c - y * s) * sc
        ref[:, blk * 32 + 16:blk * 32 + 32] = (y * c + x * s) * sc
        mag[:, blk * 32:blk * 32 + 32] = ((x.abs() + y.abs()) * sc).repeat(1, 2)
    return ref, mag


# ------------------------------------------------------------------------------------- LayerNorm fold, consumer
def fold_consumer_problem(m: int, c: int, n: int, seed: int):
    """Integer stream x [m, c] in [-15, 15] (exact in fp16; sums and sums of squares exact in fp32 for c <= 1024), gamma in
    {0.5, 1, 2}, integer W0 in [-3, 3], integer beta in [-2, 2] and b in [-8, 8]: the folded weights W0 * gamma, their column
    sums and the folded bias b + W0 . beta are exact, so the accumulator x . (W0 gamma)^T is exact in fp32."""
    g = _gen(seed)
    x = torch.randint(-15, 16, (m, c), generator=g).float()
    gam = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (c,), generator=g)]
    w0 = torch.randint(-3, 4, (n, c), generator=g).float()
    beta = torch.randint(-2, 3, (c,), generator=g).float()
    b = torch.randint(-8, 9, (n,), generator=g).float()
    wf = w0 * gam[None]
    return dict(x=x, gamma=gam, beta=beta, w0=w0, b=b, wf=wf, colsum=wf.double().sum(1).float(),
                bias=(b.double() + w0.double() @ beta.double()).float())


def fold_consumer_ref64(p, eps: float):
    """float64 LayerNorm(x) . W0^T + b written the way the fold computes it, with the magnitudes the error bound needs:
    (ref, rstd, |acc|, |mean * colsum|, kappa) - kappa = (E[x^2] + mean^2) / (var + eps) is the amplification of the
    statistics' rounding errors by the cancellation in var = E[x^2] - mean^2."""
    x = p["x"].double()
    c = x.shape[1]
    mean = x.sum(1) / c
    ex2 = (x * x).sum(1) / c
    var = ex2 - mean * mean
    rstd = 1.0 / torch.sqrt(var + eps)
    acc = x @ p["wf"].double().T
    mcs = mean[:, None] * p["colsum"].double()[None]
    ref = rstd[:, None] * (acc - mcs) + p["bias"].double()[None]
    kappa = (ex2 + mean * mean) / (var + eps)
    return ref, rstd, acc.abs(), mcs.abs(), kappa


def fold_consumer_bound(ref, rstd, acc_abs, mcs_abs, dt) -> torch.Tensor:
    """Per-element bound of the fold consumer with exact accumulator and exact statistics, e = 2^-24 (fp32 unit roundoff):
      mean = s * (1 / C)                       2 roundings                                -> 2 e on |mean|
      var + eps = fma(-mean, mean, q / C) + eps: 2 roundings of q / C, 2 x 2 e from mean^2, the fma, the add
                                               -> <= 4 e kappa relative, kappa <= 2 asserted on the inputs
      rstd = rsqrt(var + eps)                  half of that (<= 4 e) + the instruction's 1 ulp (2 e)  -> 6 e
      t = mean * colsum                        3 e on |mean colsum|
      d = acc - t,  y = rstd * d               one rounding each + rstd's 6 e              -> 8 e on |acc| + |mean colsum|
    together <= 11 e rstd (|acc| + |mean colsum|); the bound allows 16 (v_rsq_f32's accuracy is the least documented term).
    The bias add is one rounding of |ref| (2^-22 |ref| allows four), then one rounding to the output type."""
    u = torch.finfo(dt).eps / 2
    return u * ref.abs() + 16 * 2.0 ** -24 * rstd[:, None] * (acc_abs + mcs_abs) + 2.0 ** -22 * ref.abs()


def fold_consumer_f32(p, eps: float) -> torch.Tensor:
    """The fold's formula in float32 on the CPU, operation by operation (the reference alone must stay inside the bound)."""
    x = p["x"]
    c = x.shape[1]
    inv = np.float32(1.0) / np.float32(c)
    s = x.double().sum(1).float().numpy()                          # exact integer sums
    q = (x.double() ** 2).sum(1).float().numpy()
    mean = (s * inv).astype(np.float32)
    var = np.maximum((q * inv).astype(np.float32) - (mean * mean).astype(np.float32), np.float32(0)).astype(np.float32)
    rstd = (np.float32(1.0) / np.sqrt((var + np.float32(eps)).astype(np.float32))).astype(np.float32)
    acc = (x.double() @ p["wf"].double().T).float().numpy()          # exact
    t = (mean[:, None] * p["colsum"].numpy()[None]).astype(np.float32)
    y = (rstd[:, None] * (acc - t).astype(np.float32)).astype(np.float32) + p["bias"].numpy()[None]
    return torch.from_numpy(y.astype(np.float32))


# ------------------------------------------------------------------------------------------ routing attention
HD = 64


def key_codes(tk: int) -> torch.Tensor:
    """[tk, 64] float32: the 10 bits of j as -1 / +1, each repeated over 6 dimensions, then four zeros."""
    assert 1 <= tk <= 1024
    j = torch.arange(tk)
    bits = ((j[:, None] >> torch.arange(10)) & 1).float() * 2 - 1
    return torch.cat([bits.repeat_interleave(6, 1), torch.zeros(tk, 4)], 1)


PLACEMENTS = ("spread", "first", "perm")


def routing_targets(tq: int, tk: int, b: int, h: int, seed: int, placement: str = "spread") -> torch.Tensor:
    """pi [b, h, tq] (int64), its own for every batch item and head.
    "spread": every row's target is random, but rows 0, 1, 2 (mod 7) are pinned to the first key tile (keys < 64), a middle
              tile and the last (possibly partial) tile including key tk - 1;
    "first":  every target in the first key tile (the fast loop's reference maximum is the target's score itself);
    "perm":   a permutation of the keys (tq == tk)."""
    g = _gen(seed)
    if placement == "perm":
        assert tq == tk
        return torch.stack([torch.stack([torch.randperm(tk, generator=g) for _ in range(h)]) for _ in range(b)])
    if placement == "first":
        return torch.randint(0, min(64, tk), (b, h, tq), generator=g)
    assert placement == "spread"
    pi = torch.randint(0, tk, (b, h, tq), generator=g)
    nt = (tk + 63) // 64
    rows = torch.arange(tq)
    first = torch.randint(0, min(64, tk), (b, h, tq), generator=g)
    mid_lo = (nt // 2) * 64
    mid = torch.randint(mid_lo, min(mid_lo + 64, tk), (b, h, tq), generator=g)
    last_lo = (nt - 1) * 64
    last = torch.randint(last_lo, tk, (b, h, tq), generator=g)
    last[..., 2::14] = tk - 1                                            # the very last key, every other pinned row
    for r, src in ((0, first), (1, mid), (2, last)):
        sel = rows % 7 == r
        pi[..., sel] = src[..., sel]
    return pi


def routing_problem(tq: int, tk: int, b: int, h: int, seed: int, placement: str = "spread"):
    """q [b, tq, h*64] = 20 x code of the row's target, k [b, tk, h*64] = key codes (the same in every batch item and head:
    what tells batch items and heads apart is V and pi), v [b, tk, h*64] non-zero integers in +-[1, 8] (its own per batch
    item and head), pi [b, h, tq].  All values exact in bf16 and fp16."""
    g = _gen(seed + 1)
    pi = routing_targets(tq, tk, b, h, seed, placement)
    codes = key_codes(tk)
    k = codes[None, :, None, :].expand(b, tk, h, HD).reshape(b, tk, h * HD).contiguous()
    q = (20.0 * codes[pi]).permute(0, 2, 1, 3).reshape(b, tq, h * HD).contiguous()        # [b,h,tq,64] -> [b,tq,h*64]
    v = (torch.randint(1, 9, (b, tk, h * HD), generator=g) * (torch.randint(0, 2, (b, tk, h * HD), generator=g) * 2 - 1)).float()
    return q, k, v, pi


def routing_expected(v: torch.Tensor, pi: torch.Tensor, kv_batch_shift: int = 0) -> torch.Tensor:
    """[b, tq, h*64]: row i of batch item bi and head hd is V[(bi + shift) % b, pi[bi, hd, i]] of that head."""
    b, tk, c = v.shape
    h = c // HD
    vv = v.view(b, tk, h, HD).roll(-kv_batch_shift, 0)                    # item bi reads item (bi + shift) % b
    idx = pi.permute(0, 2, 1)[..., None].expand(b, pi.shape[2], h, HD)     # [b,tq,h,64]
    return torch.gather(vv, 1, idx).reshape(b, pi.shape[2], c)


def routing_gap_nats(q: torch.Tensor, k: torch.Tensor, pi: torch.Tensor, scale_nats: float) -> float:
    """Smallest margin, in nats, by which a row's target beats its best other key: float64 scores of the operands as given
    (pass the ROUNDED q for the prescaled entry point, with scale_nats = ln 2).  inf when tk == 1."""
    b, tq, c = q.shape
    tk, h = k.shape[1], c // HD
    qh = q.double().view(b, tq, h, HD).transpose(1, 2)
    kh = k.double().view(b, tk, h, HD).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) * scale_nats                            # [b,h,tq,tk]
    tgt = torch.gather(s, 3, pi[..., None])
    if tk == 1:
        return float("inf")
    rest = s.scatter(3, pi[..., None], float("-inf")).max(-1, keepdim=True).values
    return float((tgt - rest).min())


def softmax_attention64(q, k, v, scale_nats: float, kv_batch_shift: int = 0) -> torch.Tensor:
    """float64 softmax(scale q k^T) v per batch item and head, [b, tq, h*64]."""
    b, tq, c = q.shape
    tk, h = k.shape[1], c // HD
    qh = q.double().view(b, tq, h, HD).transpose(1, 2)
    kh = k.double().view(b, tk, h, HD).transpose(1, 2).roll(-kv_batch_shift, 0)
    vh = v.double().view(b, tk, h, HD).transpose(1, 2).roll(-kv_batch_shift, 0)
    o = torch.softmax(qh @ kh.transpose(-1, -2) * scale_nats, -1) @ vh
    return o.transpose(1, 2).reshape(b, tq, c)


def uniform_problem(tq: int, tk: int, b: int, h: int, seed: int):
    """q = 0: every key weighs 1 / tk (tk a power of two, so the weight and the normalisation are exact); k arbitrary small
    integers, v integers in [-8, 8].  Expected: the float64 mean of V over the keys, in every query row."""
    assert tk & (tk - 1) == 0
    g = _gen(seed)
    q = torch.zeros(b, tq, h * HD)
    k = torch.randint(-3, 4, (b, tk, h * HD), generator=g).float()
    v = torch.randint(-8, 9, (b, tk, h * HD), generator=g).float()
    return q, k, v


def uniform_expected64(v: torch.Tensor, tq: int, kv_batch_shift: int = 0) -> torch.Tensor:
    return v.double().roll(-kv_batch_shift, 0).mean(1, keepdim=True).expand(-1, tq, -1)


# ---------------------------------------------------------------------------------------------------- checker
def ulp_step(x: torch.Tensor) -> torch.Tensor:
    """x moved by one unit in the last place of its own type, away from zero (x finite, of a 16-bit type or float32)."""
    it = {2: torch.int16, 4: torch.int32}[x.element_size()]
    return (x.contiguous().view(it) + 1).view(x.dtype)


def assert_equal_elementwise(out: torch.Tensor, ref: torch.Tensor, what: str, max_report: int = 8):
    """`out` must equal `ref` element for element (ref is cast to out's dtype first: one round to nearest even when it is the
    float64 result).  On failure: how many elements differ and the first few as (row, column, got, expected) with
    row % 256 / column % 256, so the tile position is readable.  Leading dimensions are folded into the row."""
    assert tuple(out.shape) == tuple(ref.shape), f"{what}: shape {tuple(out.shape)} vs {tuple(ref.shape)}"
    exp = ref.to(device=out.device).to(out.dtype)
    if torch.equal(out, exp):
        return
    cols = out.shape[-1] if out.dim() else 1
    o2, e2 = out.reshape(-1, cols), exp.reshape(-1, cols)
    bad = (o2 != e2) | (torch.isnan(o2) != torch.isnan(e2))
    idx = bad.nonzero()
    nbad = int(idx.shape[0])
    rows_bad = int(bad.any(1).sum())
    cols_bad = int(bad.any(0).sum())
    lines = []
    for r, c in idx[:max_report].tolist():
        lines.append(f"  row {r} (%256 = {r % 256}) col {c} (%256 = {c % 256}): got {float(o2[r, c])!r} expected {float(e2[r, c])!r}")
    raise AssertionError(f"{what}: {nbad} of {o2.numel()} elements differ ({rows_bad} rows, {cols_bad} columns touched); first "
                         f"{len(lines)}:\n" + "\n".join(lines))


def assert_within(out: torch.Tensor, ref64: torch.Tensor, bound: torch.Tensor, what: str, max_report: int = 8):
    """|out - ref64| <= bound per element (float64 on out's device); same report as assert_equal_elementwise."""
    d = (out.double() - ref64.to(out.device)).abs()
    bnd = bound.to(out.device)
    bad = ~(d <= bnd)
    if not bool(bad.any()):
        return
    cols = out.shape[-1]
    idx = bad.reshape(-1, cols).nonzero()
    o2, r2, d2, b2 = out.reshape(-1, cols), ref64.to(out.device).reshape(-1, cols), d.reshape(-1, cols), bnd.reshape(-1, cols)
    lines = [f"  row {r} (%256 = {r % 256}) col {c} (%256 = {c % 256}): got {float(o2[r, c])!r} expected {float(r2[r, c])!r} "
             f"|diff| {float(d2[r, c]):.3e} > bound {float(b2[r, c]):.3e}" for r, c in idx[:max_report].tolist()]
    raise AssertionError(f"{what}: {int(idx.shape[0])} of {out.numel()} elements outside their bound; worst diff / bound = "
                         f"{float((d / bnd).max()):.3f}; first {len(lines)}:\n" + "\n".join(lines))
