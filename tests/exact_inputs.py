"""Inputs for which the correct answer of a kernel is EXACT, and an element-wise checker.

Three constructions ("Exact-input tests"):

* integer GEMM: operands, bias and residual hold small integers (or integers times a power of two), so every product and
  every partial sum is an integer below 2^24: fp32 accumulation is exact in ANY order, on any tile shape.  The kernel must
  return the float64 result rounded once to the output type, bit for bit.
* routing attention: key j carries the code of j's 10 bits in {-1, +1}, query i is 20 x the code of its target pi(i).  The
  target's score beats every other key's by >= 30 nats, so the softmax row is (1, 0, ...) to below 2^-24 and the output row
  must be V[pi(i)] bit for bit.
* power-of-two softmax: one-hot keys and integer query tables make every score one exact product and every softmax weight
  2^(s - m) an exact power of two; row profiles prescribe the maximum of each key tile, so each rescale branch of the
  attention kernels runs on known rows, and the weighted sum is compared element-wise with float64 under a derived bound.

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


# ------------------------------------------------------------------------------- power-of-two softmax weights
# Row profiles: what a query row prescribes as the maximum of each key tile (64 keys), relative to its first tile.
POW2_PROFILES = ("flat", "stair", "jump", "fall", "keeper", "keeper-last", "keeper-twice", "tail-max", "ripple")
POW2_OVERFLOW = ("overflow-l", "overflow-inf")
POW2_ALL = POW2_PROFILES + POW2_OVERFLOW
# key tiles a profile needs to exist; with fewer the row is "flat" (and recorded as flat: see pow2_profile_ids)
POW2_MIN_TILES = {"flat": 1, "stair": 2, "jump": 2, "fall": 2, "keeper": 3, "keeper-last": 2, "keeper-twice": 6, "tail-max": 1,
                  "ripple": 2, "overflow-l": 2, "overflow-inf": 2}
POW2_VARIANTS = ("mixed", "banded", "overflow")
POW2_TAIL_MAX = 5                                # the lone last key of a tail-max row, above every other key's tile offset


def pow2_profile_ids(tq: int, tk: int, b: int, h: int, variant: str):
    """(prof, kpos), both int64 [b, h, tq]: index into POW2_ALL and the counter that places a profile's event tile.
    mixed:    prof = (row + head + batch) % P - every 16-row query tile holds every profile; kpos = row // P.
    banded:   prof = (row // 32 + head + batch) % P - a wave holds ONE profile in both workgroup shapes, and with
              kpos = row // 32 all its rows meet the event in the same tile.
    overflow: mixed, but rows < 64 of even heads run over POW2_ALL (the two overflow profiles included).
    A profile that needs more key tiles than ceil(tk / 64) becomes flat HERE, so the ids say what the rows really are."""
    p, nt = len(POW2_PROFILES), (tk + 63) // 64
    row, head, bat = torch.arange(tq)[None, None, :], torch.arange(h)[None, :, None], torch.arange(b)[:, None, None]
    zero = torch.zeros(b, h, tq, dtype=torch.int64)
    if variant == "banded":
        prof, kpos = (row // 32 + head + bat) % p, row // 32 + zero
    else:
        assert variant in ("mixed", "overflow")
        prof, kpos = (row + head + bat) % p, row // p + zero
        if variant == "overflow":
            sel = ((row < 64) & (head % 2 == 0)).expand(b, h, tq)
            prof = torch.where(sel, (row + head + bat) % len(POW2_ALL), prof)
            kpos = torch.where(sel, row // len(POW2_ALL) + zero, kpos)
    need = torch.tensor([POW2_MIN_TILES[n] for n in POW2_ALL])
    return torch.where(need[prof] <= nt, prof, torch.zeros_like(prof)), kpos


def pow2_problem(tq: int, tk: int, b: int, h: int, seed: int, variant: str = "mixed"):
    """Attention inputs whose every softmax weight is an exact power of two.
      k [b, tk, h*64]  one-hot: key j has the class 4 * slot + sub, slot = (j // 64) % 16 (its key tile, tk <= 1024) and sub in
                       0..3 - its own random layout per batch item and head, each sub 16 times per full tile; in the last tile
                       key tk - 1 ALONE has sub 3 (the others 0..2), so a row can single it out;
      q [b, tq, h*64]  a table of 64 integers per row and head: q[4 * slot + sub] = off[slot] - lvl[slot][sub] + shift, with off
                       the profile's tile offsets, lvl a random permutation of 0..3 per row and slot (a spread of 0..3 below the
                       tile's maximum) and shift a per-row integer that centres the table in [-127, 127] (+ a jitter of +-5);
      v                as routing_problem: non-zero integers in +-[1, 8], its own per batch item and head.
    The score s_ij = q_i . k_j = q_i[class_j] is ONE non-zero product: exact in the matrix core in any order, and with an
    exp2 softmax (prescaled entry points as they are, classic ones at scale = ln 2) every weight 2^(s - m) is a power of two
    whatever reference m the kernel holds.  Tile offsets per profile (event tiles move with kpos; t = tile, nt = tiles):
      flat 0 | stair 3 (t - nt + 1) on the last four tiles, 36 lower (still climbing by 3) before | jump +40 in one tile > 0 |
      fall 0, then -30 | keeper +70 in a tile that is neither first nor last | keeper-last +70 in the last | keeper-twice
      +70 in tile 1 or 2, +135 in tile nt - 2 or nt - 3 | tail-max 0, key tk - 1 at +POW2_TAIL_MAX | ripple (3 t + row) % 6 |
      overflow-l +105 / overflow-inf +140 in one tile > 0.
    Returns q, k, v (float32 holders, exact in bf16 and fp16) and info = dict(prof, table [b,h,tq,64] (= q per head), cls
    [b,h,tk])."""
    assert 1 <= tk <= 1024
    g = _gen(seed)
    nt = (tk + 63) // 64
    prof, kpos = pow2_profile_ids(tq, tk, b, h, variant)
    idx = {n: i for i, n in enumerate(POW2_ALL)}
    t = torch.arange(16)[None, None, None, :]
    pr, kp = prof[..., None], kpos[..., None]
    row = torch.arange(tq)[None, None, :, None]
    tl = t - (nt - 1)
    at = lambda pos: (t == pos).long()
    anywhere = 1 + kp % max(nt - 1, 1)                                    # a tile that is not the first
    inner = 1 + kp % max(nt - 2, 1)                                       # ... nor the last
    offs = {
        "stair": torch.where(tl >= -3, 3 * tl, 3 * (tl + 4) - 36),
        "jump": 40 * at(anywhere),
        "fall": -30 * (t > 0).long(),
        "keeper": 70 * at(inner),
        "keeper-last": 70 * at(nt - 1),
        "keeper-twice": 70 * at(1 + kp % 2) + 135 * at(nt - 2 - (kp // 2) % 2),
        "ripple": (3 * t + row) % 6,
        "overflow-l": 105 * at(anywhere),
        "overflow-inf": 140 * at(anywhere),
    }
    off = torch.zeros(b, h, tq, 16, dtype=torch.int64)
    for name, o in offs.items():
        off = torch.where(pr == idx[name], o.expand_as(off), off)
    off = torch.where(t < nt, off, torch.zeros_like(off))                 # slots without a key tile: never read
    lvl = torch.rand(b, h, tq, 16, 4, generator=g).argsort(-1)
    table = off[..., None] - lvl                                          # [b,h,tq,16,4]
    tm = prof == idx["tail-max"]
    table[..., nt - 1, 3] = torch.where(tm, torch.full_like(prof, POW2_TAIL_MAX), table[..., nt - 1, 3])
    table = table.reshape(b, h, tq, 64)
    hi, lo = table.amax(-1, keepdim=True), table.amin(-1, keepdim=True)
    table = table - (hi + lo) // 2 + torch.randint(-5, 6, (b, h, tq, 1), generator=g)
    assert int(table.abs().max()) <= 127
    q = table.permute(0, 2, 1, 3).reshape(b, tq, h * HD).float().contiguous()
    sub = (torch.rand(b, h, 16, 64, generator=g).argsort(-1) % 4).reshape(b, h, 1024)[..., :tk].contiguous()
    last = (nt - 1) * 64
    sub[..., last:] = sub[..., last:] % 3
    sub[..., tk - 1] = 3
    cls = (torch.arange(tk) // 64 % 16) * 4 + sub                         # [b,h,tk]
    k = torch.nn.functional.one_hot(cls, 64).float().permute(0, 2, 1, 3).reshape(b, tk, h * HD).contiguous()
    v = (torch.randint(1, 9, (b, tk, h * HD), generator=g) * (torch.randint(0, 2, (b, tk, h * HD), generator=g) * 2 - 1)).float()
    return q, k, v, dict(prof=prof, table=table, cls=cls)


def pow2_scores(q: torch.Tensor, k: torch.Tensor, kv_batch_shift: int = 0) -> torch.Tensor:
    """float64 q k^T per batch item and head, [b, h, tq, tk] (integers: exact); item bi reads the keys of (bi + shift) % b."""
    b, tq, c = q.shape
    tk, h = k.shape[1], c // HD
    qh = q.double().view(b, tq, h, HD).transpose(1, 2)
    kh = k.double().view(b, tk, h, HD).transpose(1, 2).roll(-kv_batch_shift, 0)
    return qh @ kh.transpose(-1, -2)


def pow2_tile_maxima(s: torch.Tensor) -> torch.Tensor:
    """[..., tq, nt]: the largest score of every 64-key tile."""
    tk = s.shape[-1]
    nt = (tk + 63) // 64
    sp = torch.nn.functional.pad(s, (0, nt * 64 - tk), value=float("-inf"))
    return sp.reshape(s.shape[:-1] + (nt, 64)).amax(-1)


def pow2_exponent_error(s: torch.Tensor) -> torch.Tensor:
    """E_cls per row [..., tq] for the classic entry points launched at scale = ln 2: they form the exp2 argument as
    fma32(s, c32, -float32(m * c32)) with c32 = float32(float32(ln 2) * 1.4426950408889634f) (the product rounded on its own
    in one score per tile: both forms are evaluated), where the argument meant is s - m.  Largest deviation over the row's
    keys and over m in the row's tile maxima (every running maximum is one of them), times ln 2 (d 2^x = ln 2 2^x dx, and
    2^x <= 1), times 2 for margin.  Computed from the problem alone; float32 fma through float64, as _fma32 of the CPU tests."""
    c32 = float(np.float32(np.float32(math.log(2.0)) * np.float32(1.4426950408889634)))
    m = pow2_tile_maxima(s)                                               # [..., tq, nt]
    mb = (m * c32).float().double()[..., None, :]                         # float32(m * c32)
    sx = s[..., :, None]                                                  # [..., tq, tk, 1]
    want = sx - m[..., None, :]
    fused = (sx * c32 - mb).float().double()
    split = ((sx * c32).float().double() - mb).float().double()
    err = torch.maximum((fused - want).abs(), (split - want).abs())
    return 2.0 * math.log(2.0) * err.amax((-1, -2))


def pow2_reference(q, k, v, kv_batch_shift: int = 0, classic: bool = False):
    """float64 reference of the power-of-two problem on the tensors' device, sharing no code with the kernel:
    w_j = 2^(s_j - M), ref = sum w v / sum w, A = sum w |v| / sum w.  Returns dict(ref, A [b,tq,h*64], narrow (all of the
    row's log2-weights in [-8, 0]), gap_ok (every log2-weight in [-12, 0] or <= -30), ecls (pow2_exponent_error, or zeros
    unless classic) - the last three [b,tq,h*64] as well, constant over a head's 64 columns)."""
    b, tq, c = q.shape
    tk, h = k.shape[1], c // HD
    s = pow2_scores(q, k, kv_batch_shift)
    d = s - s.amax(-1, keepdim=True)
    w = torch.exp2(d)
    vh = v.double().view(b, tk, h, HD).transpose(1, 2).roll(-kv_batch_shift, 0)
    den = w.sum(-1, keepdim=True)
    cols = lambda x: x.transpose(1, 2).reshape(b, tq, c)                  # [b,h,tq,64] -> [b,tq,h*64]
    rows = lambda x: cols(x[..., None].expand(b, h, tq, HD))              # [b,h,tq]    -> [b,tq,h*64]
    ecls = pow2_exponent_error(s) if classic else torch.zeros_like(den[..., 0])
    return dict(ref=cols(w @ vh / den), A=cols(w @ vh.abs() / den), narrow=rows(d.amin(-1) >= -8),
                gap_ok=rows(((d >= -12) | (d <= -30)).all(-1)), ecls=rows(ecls))


def pow2_allowance(r: dict, tk: int) -> torch.Tensor:
    """t, the allowance for the kernel's fp32 arithmetic, relative to A = sum w |v| / sum w (e = 2^-24):
        t = c e A + 2 E_cls A
    narrow rows (all log2-weights in [-8, 0]; tk <= 1024, |v| <= 8): every partial sum of l (<= 2^10, multiples of 2^-8 of the
      largest weight) and of o (<= 2^13) fits in 22 bits, so both accumulate EXACTLY in any order under any lagging
      reference (a change of reference is a power of two).  c = 8: l built from unrounded exp2 outputs of 1 ulp each where the
      kernel sums them on the VALU (2), 1 / l (2), the product o * (1 / l) (1), slack (3).
    other rows: c = tk + 8 - one fp32 rounding per accumulated key (the matrix core's internal order is not documented).
    E_cls: pow2_exponent_error, zero for the prescaled entry points; it moves every weight by at most a factor 1 +- E_cls,
      hence numerator and denominator by E_cls A each."""
    c = torch.where(r["narrow"], torch.full_like(r["A"], 8.0), torch.full_like(r["A"], tk + 8.0))
    return c * 2.0 ** -24 * r["A"] + 2.0 * r["ecls"] * r["A"]


def pow2_bound(r: dict, tk: int, dt) -> torch.Tensor:
    """Per-element bound: one rounding to the output type of a value within t of ref, u (|ref| + t) + t."""
    t = pow2_allowance(r, tk)
    return torch.finfo(dt).eps / 2 * (r["ref"].abs() + t) + t


def pow2_online_softmax_f32(s: torch.Tensor, vh: torch.Tensor, reverse: bool = False) -> torch.Tensor:
    """The plain online softmax in float32 on the CPU, one key at a time with a per-key running maximum (numpy, operation by
    operation): m' = max(m, s_j), alpha = 2^(m - m'), p = 2^(s_j - m'), l = l alpha + p, o = o alpha + p v_j; out = o / l.
    s [b,h,tq,tk] integers, vh [b,h,tk,64]; keys in reversed order if asked.  Returns float32 [b,h,tq,64], not rounded."""
    sn, vn = s.numpy().astype(np.float32), vh.numpy().astype(np.float32)
    b, h, tq, tk = sn.shape
    m = np.full((b, h, tq), -np.inf, np.float32)
    l = np.zeros((b, h, tq), np.float32)
    o = np.zeros((b, h, tq, HD), np.float32)
    with np.errstate(invalid="ignore"):
        for j in (range(tk - 1, -1, -1) if reverse else range(tk)):
            mn = np.maximum(m, sn[..., j])
            alpha = np.exp2(m - mn).astype(np.float32)
            p = np.exp2(sn[..., j] - mn).astype(np.float32)
            l = (l * alpha).astype(np.float32) + p
            o = (o * alpha[..., None]).astype(np.float32) + (p[..., None] * vn[:, :, None, j, :]).astype(np.float32)
            m = mn
    return torch.from_numpy((o / l[..., None]).astype(np.float32))


# ------------------------------------------------------------------------------------------ integer convolution
def int_conv(b: int, h: int, w: int, cin: int, cout: int, seed: int, groups: int = 1):
    """x [groups, b, h, w, cin] in [-3, 3] with a few -0.0, W [groups, cout, 3, 3, cin] in [-3, 3], bias [groups, cout] in
    [-64, 64]: float32 holders of integers, exact in bf16 and fp16, its own weights and bias per group.  With cin <= 256 every
    partial sum of conv + bias + residual (integers in [-64, 64]) stays below 9 * 256 * 9 + 128 < 2^24: fp32 accumulation is
    exact in any order - per tap, per channel slice, per split-K plane."""
    assert cin <= 256
    g = _gen(seed)
    x = torch.randint(-3, 4, (groups, b, h, w, cin), generator=g).float()
    wt = torch.randint(-3, 4, (groups, cout, 3, 3, cin), generator=g).float()
    bias = torch.randint(-64, 65, (groups, cout), generator=g).float()
    flat = x.view(-1)
    flat[torch.randint(0, flat.numel(), (max(4, flat.numel() // 97),), generator=g)] = -0.0
    return x, wt, bias


def tap_identity_weights(cout: int, cin: int, single_tap: bool = False) -> torch.Tensor:
    """[cout, 3, 3, cin]: w[co, ky, kx, ci] = 1 where ci == (co + 7 * (3 ky + kx)) % cin, else 0 - output channel co is the sum
    of nine known shifted input channels, one per tap.  single_tap: only tap co % 9 is kept, so output (y, x, co) is ONE input
    element (or the zero padding)."""
    co = torch.arange(cout)[:, None]
    t = torch.arange(9)[None, :]
    ci = (co + 7 * t) % cin                                               # [cout, 9]
    w = torch.zeros(cout, 9, cin)
    w.scatter_(2, ci[..., None], 1.0)
    if single_tap:
        w = w * (t == co % 9).float()[..., None]
    return w.view(cout, 3, 3, cin)


def conv_out_size(h: int, w: int, stride: int = 1):
    return (h + 2 - 3) // stride + 1, (w + 2 - 3) // stride + 1


def conv_cols(x: torch.Tensor, stride: int = 1) -> torch.Tensor:
    """x [..., b, h, w, c] -> [..., b * oh * ow, 9 c]: nine shifted (strided) slices of the zero-padded map, concatenated in
    (ky, kx, ci) order - the layout of W [cout, 3, 3, cin] flattened to [cout, 9 cin]."""
    h, w, c = x.shape[-3:]
    oh, ow = conv_out_size(h, w, stride)
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    sl = [xp[..., ky:ky + stride * (oh - 1) + 1:stride, kx:kx + stride * (ow - 1) + 1:stride, :] for ky in range(3) for kx in range(3)]
    return torch.cat(sl, -1).reshape(x.shape[:-4] + (x.shape[-4] * oh * ow, 9 * c))


def conv_ref64(x, w, bias=None, resid=None, stride: int = 1, relu_input: bool = False, dtype=torch.float64) -> torch.Tensor:
    """3x3 convolution, padding 1, of x [..., b, h, w, cin] with w [..., cout, 3, 3, cin] (+ bias [..., cout]) (+ resid
    [..., b, oh, ow, cout]) -> [..., b, oh, ow, cout] in float64, as shifted slices fed through gemm_ref64: no convolution
    library, no code shared with the kernels.  relu_input: x is clamped at 0 first.  dtype=torch.float32 is for integer inputs
    only, where a float32 matmul is exact as well."""
    b, h, wd, cin = x.shape[-4:]
    oh, ow = conv_out_size(h, wd, stride)
    cout = w.shape[-4]
    xx = x.to(dtype)
    if relu_input:
        xx = xx.clamp(min=0)
    cols = conv_cols(xx, stride)
    wf = w.to(dtype).reshape(w.shape[:-4] + (cout, 9 * cin))
    if dtype == torch.float64:
        ref = gemm_ref64(cols, wf, bias)
    else:
        ref = cols @ wf.transpose(-1, -2)
        if bias is not None:
            ref = ref + bias.to(dtype).unsqueeze(-2)
    ref = ref.reshape(x.shape[:-4] + (b, oh, ow, cout))
    if resid is not None:
        ref = ref + resid.to(dtype)
    return ref


def conv_max_partial_sum(x, w, bias=None, resid_lim: int = 64, stride: int = 1) -> float:
    """Upper bound of every partial sum any summation order can form: sum of |x| |w| over the window + |bias| + resid_lim."""
    m = conv_ref64(x.abs(), w.abs(), None if bias is None else bias.abs(), stride=stride)
    return float(m.max()) + resid_lim


# ----------------------------------------------------------------------------------------------- fused head tail
def head4_problem(b: int, h: int, w: int, cin: int, seed: int, groups: int = 1, zero_patches: int = 3):
    """Inputs of the fused head tail relu(conv3x3(x) + bias) [128 channels, fp32 registers] -> W4 [4, 128], b4 -> (xyz, logit)
    for which r = [xyz, logit] is EXACT in fp32:
      x      integers in [-a, a], the amplitude a in {1, 2, 3} constant on 4 x 4 blocks (so |xyz| spreads over (0, 6]), and
             `zero_patches` 5 x 5 patches of zeros per image (the first in the corner (0, 0)): the pixels whose whole window is
             zero have h = relu(bias);
      w      sparse: three taps of +-1 per output channel; bias integers in [-2, 1]: h is an integer in [0, 10];
      W4     integers in [-8, 8] times 2^-7 (xyz rows) / 2^-6 (logit row); b4 multiples of 2^-7, chosen so that
             xyz = relu(bias) . W4^T + b4 = 0 exactly on the all-zero windows (the 1e-8 clamp branch); logit bias in [-1, 1].
    Every product h * W4 is a multiple of 2^-7 below 2^0, every sum of 128 of them below 2^7: 14 bits, exact in any order."""
    g = _gen(seed)
    amp = torch.randint(1, 4, (groups, b, (h + 3) // 4, (w + 3) // 4, 1), generator=g)
    amp = amp.repeat_interleave(4, 2).repeat_interleave(4, 3)[:, :, :h, :w]
    x = (torch.randint(-3, 4, (groups, b, h, w, cin), generator=g).clamp(-amp, amp)).float()
    for gi in range(groups):
        for bi in range(b):
            for k in range(zero_patches):
                y0 = 0 if k == 0 else int(torch.randint(0, max(1, h - 4), (1,), generator=g))
                x0 = 0 if k == 0 else int(torch.randint(0, max(1, w - 4), (1,), generator=g))
                x[gi, bi, y0:y0 + 5, x0:x0 + 5] = 0.0
    wt = torch.zeros(groups, 128, 9 * cin)
    idx = torch.rand(groups, 128, 9 * cin, generator=g).argsort(-1)[..., :3]
    wt.scatter_(-1, idx, (torch.randint(0, 2, (groups, 128, 3), generator=g) * 2 - 1).float())
    wt = wt.view(groups, 128, 3, 3, cin)
    bias = torch.randint(-2, 2, (groups, 128), generator=g).float()
    w4 = torch.randint(-8, 9, (groups, 4, 128), generator=g).float() * 2.0 ** -7
    w4[:, 3] *= 2.0
    b4 = torch.zeros(groups, 4)
    b4[:, :3] = -(torch.relu(bias).double()[:, None, :] * w4[:, :3].double()).sum(-1).float()
    b4[:, 3] = torch.randint(-128, 129, (groups,), generator=g).float() * 2.0 ** -7
    return dict(x=x, w=wt, bias=bias, w4=w4, b4=b4)


def head4_r64(p, x=None, use_bias: bool = True) -> torch.Tensor:
    """float64 r = relu(conv(x) + bias) . W4^T + b4, [groups, b, h, w, 4]; x: another input map for the same weights."""
    hmap = torch.relu(conv_ref64(p["x"] if x is None else x, p["w"], p["bias"] if use_bias else None))
    return hmap @ p["w4"].double().transpose(-1, -2)[:, None, None] + p["b4"].double()[:, None, None, None, :]


def head4_expected64(r64: torch.Tensor):
    """pts = xyz / max(|xyz|, 1e-8) * expm1(|xyz|), conf = 1 + exp(logit), float64."""
    xyz, c = r64[..., :3], r64[..., 3]
    d = xyz.norm(dim=-1, keepdim=True)
    return xyz / d.clamp(min=1e-8) * torch.expm1(d), 1.0 + torch.exp(c)


def exp_f32_errors(r64: torch.Tensor):
    """(E_expm1, E_exp): RELATIVE error of float32 numpy expm1 at d = float32(|xyz|) and exp at the logit against float64 at
    the same float32 argument, maximum over the problem's own r values, times 4 - the margin for the device's expm1f / expf,
    whose accuracy is not documented.  Measured on the reference side only, like rope_trig_error."""
    xyz = r64[..., :3].double().numpy()
    d32 = np.sqrt((xyz * xyz).sum(-1)).astype(np.float32)
    d32 = d32[d32 > 0]
    c32 = r64[..., 3].numpy().astype(np.float32)
    e1 = np.abs(np.expm1(d32).astype(np.float64) - np.expm1(d32.astype(np.float64))) / np.expm1(d32.astype(np.float64))
    e2 = np.abs(np.exp(c32).astype(np.float64) - np.exp(c32.astype(np.float64))) / np.exp(c32.astype(np.float64))
    return 4.0 * float(e1.max()), 4.0 * float(e2.max())


def head4_bounds(r64: torch.Tensor, e_expm1: float, e_exp: float):
    """Per-element bounds of the tail at an exact r = (x, y, z, c), e = 2^-24, from the kernels' formula
        d = sqrtf(x x + y y + z z);  sc = expm1f(d) / fmaxf(d, 1e-8f);  pts = (x, y, z) * sc;  conf = 1 + expf(c):
      s = x x + y y + z z   three non-negative terms, each product and each of the two sums rounded (or fused): <= 3 e relative
      d = sqrtf(s)          half of that + the root's own rounding (2 e allowed)                                -> 4 e on d
      E = expm1f(d)         the argument's error amplified by kappa(d) = d e^d / (e^d - 1) (in [1, d + 1)): 4 e kappa,
                            plus the function's own error e_expm1 (measured, exp_f32_errors)
      sc = E / d            d's 4 e again + the division (2 e allowed);  pts = x * sc: one rounding
    pts:  |ref| ((4 kappa + 7) e + e_expm1).   d = 0: expm1f(0) = 0, sc = 0, pts = 0 exactly - the bound is 0 there.
    conf: e_exp exp(c) + 2 e (1 + exp(c)) - the function's error and the rounding of the sum (one rounding; two allowed)."""
    e = 2.0 ** -24
    xyz, c = r64[..., :3], r64[..., 3]
    d = xyz.norm(dim=-1, keepdim=True)
    kappa = torch.where(d > 0, d * torch.exp(d) / torch.expm1(d).clamp(min=1e-300), torch.ones_like(d))
    pts, conf = head4_expected64(r64)
    return pts.abs() * ((4 * kappa + 7) * e + e_expm1), e_exp * torch.exp(c) + 2 * e * (1 + torch.exp(c))


def head4_f32(r64: torch.Tensor):
    """The tail's formula in float32 on the CPU, operation by operation (numpy)."""
    r = r64.numpy().astype(np.float32)
    assert np.array_equal(r.astype(np.float64), r64.numpy())
    x, y, z, c = r[..., 0], r[..., 1], r[..., 2], r[..., 3]
    s = ((x * x).astype(np.float32) + (y * y).astype(np.float32)).astype(np.float32) + (z * z).astype(np.float32)
    d = np.sqrt(s.astype(np.float32)).astype(np.float32)
    sc = (np.expm1(d).astype(np.float32) / np.maximum(d, np.float32(1e-8))).astype(np.float32)
    pts = np.stack([x * sc, y * sc, z * sc], -1).astype(np.float32)
    conf = (np.float32(1.0) + np.exp(c).astype(np.float32)).astype(np.float32)
    return torch.from_numpy(pts), torch.from_numpy(conf)


# ------------------------------------------------------------------------------------ x2 align-corners upsample
def const_map(b: int, h: int, w: int, c: int, seed: int, groups: int = 1):
    """v [groups, b, c] integers in [-3, 3] (its own per group, batch item and channel) and the map x[g, b, :, :, c] = v."""
    v = torch.randint(-3, 4, (groups, b, c), generator=_gen(seed)).float()
    return v, v[:, :, None, None, :].expand(groups, b, h, w, c).contiguous()


def quarter_values(shape, seed: int) -> torch.Tensor:
    """Multiples of 1/4 within [-4, 4]: 6 bits, exact in bf16 and fp16."""
    return torch.randint(-16, 17, tuple(shape), generator=_gen(seed)).float() / 4.0


def upsample_coords_f32(n_in: int, n_out: int, n_full: int = 0):
    """The kernels' coordinate arithmetic in float32 for output indices 0 .. n_out - 1 of the FULL x2 map (n_full = 2 n_in):
    s = (float)(n_in - 1) / (float)(n_full - 1), f = i * s, i0 = min((int) f, n_in - 1), i1 = min(i0 + 1, n_in - 1), w = f - i0.
    Returns (i0, i1, w) as numpy arrays (w float32)."""
    n_full = n_full or 2 * n_in
    s = np.float32(n_in - 1) / np.float32(n_full - 1) if n_full > 1 else np.float32(0)
    f = (np.arange(n_out).astype(np.float32) * s).astype(np.float32)
    i0 = np.minimum(f.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, (f - i0.astype(np.float32)).astype(np.float32)


def blend_f32(a, b, w):
    """a * (1 - w) + b * w in float32, operation by operation (numpy float32 arrays)."""
    one_m = (np.float32(1) - w).astype(np.float32)
    return ((a * one_m).astype(np.float32) + (b * w).astype(np.float32)).astype(np.float32)


def upsample2x_f32(x: torch.Tensor, oh: int = 0, ow: int = 0) -> torch.Tensor:
    """The kernels' x2 upsample of x [..., h, w, c] in float32 on the CPU: float32 coordinates, horizontal blends, then the
    vertical blend; cropped to (oh, ow).  Not rounded to 16 bits."""
    h, w = x.shape[-3:-1]
    oh, ow = oh or 2 * h, ow or 2 * w
    y0, y1, wy = upsample_coords_f32(h, oh)
    x0, x1, wx = upsample_coords_f32(w, ow)
    xn = x.numpy().astype(np.float32)
    wxb, wyb = wx[:, None], wy[:, None, None]
    top = blend_f32(xn[..., y0, :, :][..., :, x0, :], xn[..., y0, :, :][..., :, x1, :], wxb)
    bot = blend_f32(xn[..., y1, :, :][..., :, x0, :], xn[..., y1, :, :][..., :, x1, :], wxb)
    return torch.from_numpy(blend_f32(top, bot, wyb))


def _nbr_max(d: torch.Tensor, dim: int) -> torch.Tensor:
    """max over positions i - 1, i, i + 1 along dim."""
    n = d.shape[dim]
    lo = torch.cat([d.narrow(dim, 0, 1), d.narrow(dim, 0, n - 1)], dim)
    hi = torch.cat([d.narrow(dim, 1, n - 1), d.narrow(dim, n - 1, 1)], dim)
    return torch.maximum(d, torch.maximum(lo, hi))


def upsample2x_ref64(x: torch.Tensor, oh: int = 0, ow: int = 0):
    """float64 bilinear x2 upsample (align_corners) of x [..., h, w, c] with the EXACT weights: output index i reads source
    coordinate i (n - 1) / (2 n - 1).  Returns (ref, t): t is the allowance for the kernels' fp32 arithmetic,
        t = 2^-23 h Sy + 2^-23 w Sx + 16 * 2^-24 A:
    the coordinate f = i * s carries two roundings (s, then the product), at most 2^-23 n absolute; the blend is continuous and
    piecewise linear, so a coordinate error moves the value by at most the error times the local slope - Sy / Sx = the
    largest |difference of vertically / horizontally adjacent source pixels| over the cell and its neighbours (a floor that
    lands on the other side of an integer evaluates the neighbouring cell, at a weight within 2^-23 n of 0 or 1); the three
    blends are <= 8 roundings relative to A = the largest |corner| (16 allowed, FMA contraction included)."""
    h, w = x.shape[-3:-1]
    oh, ow = oh or 2 * h, ow or 2 * w
    xd = x.double()

    def coords(n, n_out):
        f = torch.arange(n_out, dtype=torch.float64) * (n - 1) / (2 * n - 1)
        i0 = f.floor().long().clamp(max=n - 1)
        return i0, (i0 + 1).clamp(max=n - 1), f - i0
    y0, y1, wy = coords(h, oh)
    x0, x1, wx = coords(w, ow)
    rows = lambda t, i: t.index_select(-3, i)
    cols = lambda t, i: t.index_select(-2, i)
    wxb, wyb = wx[:, None], wy[:, None, None]
    top = cols(rows(xd, y0), x0) * (1 - wxb) + cols(rows(xd, y0), x1) * wxb
    bot = cols(rows(xd, y1), x0) * (1 - wxb) + cols(rows(xd, y1), x1) * wxb
    ref = top * (1 - wyb) + bot * wyb
    zy, zx = torch.zeros_like(xd[..., :1, :, :]), torch.zeros_like(xd[..., :, :1, :])
    dy = torch.cat([(xd[..., 1:, :, :] - xd[..., :-1, :, :]).abs(), zy], -3)      # dy[y] = |x[y + 1] - x[y]| (0 in the last row)
    dx = torch.cat([(xd[..., :, 1:, :] - xd[..., :, :-1, :]).abs(), zx], -2)
    sy = _nbr_max(_nbr_max(dy, -3), -2)                                              # over the cell's two columns and row neighbours
    sx = _nbr_max(_nbr_max(dx, -2), -3)
    amax = _nbr_max(_nbr_max(xd.abs(), -3), -2)
    g = lambda t: cols(rows(t, y0), x0)
    t = 2.0 ** -23 * (h * g(sy) + w * g(sx)) + 16 * 2.0 ** -24 * g(amax)
    return ref, t


def upsample_bound(ref64: torch.Tensor, t: torch.Tensor, dt) -> torch.Tensor:
    """One rounding to the 16-bit type of a value within t of ref64: u (|ref| + t) + t, or half the spacing of the type's
    subnormals where that is larger (2^-25 in fp16: a blend may cancel to below 2^-14)."""
    fi = torch.finfo(dt)
    return (fi.eps / 2 * (ref64.abs() + t)).clamp(min=fi.smallest_normal * fi.eps / 2) + t


def single_tap_gather(m: torch.Tensor, cout: int) -> torch.Tensor:
    """What a convolution with tap_identity_weights(cout, cin, single_tap=True) makes of the map m [..., h, w, cin]: output
    (y, x, co) = m[y + ky - 1, x + kx - 1, (co + 7 t) % cin] with t = co % 9 = 3 ky + kx, zero outside the map."""
    h, w, cin = m.shape[-3:]
    mp = torch.nn.functional.pad(m, (0, 0, 1, 1, 1, 1))
    out = []
    for co in range(cout):
        t = co % 9
        out.append(mp[..., t // 3:t // 3 + h, t % 3:t % 3 + w, (co + 7 * t) % cin])
    return torch.stack(out, -1)


# ---------------------------------------------------------------------------------------------------- checker
def ulp_step(x: torch.Tensor) -> torch.Tensor:
    """x moved by one unit in the last place of its own type, away from zero (x finite, of a 16-bit type or float32)."""
    it = {2: torch.int16, 4: torch.int32}[x.element_size()]
    return (x.contiguous().view(it) + 1).view(x.dtype)


def _where(r: int, c: int, hw) -> str:
    """Position of element (row r, column c) in a report; hw = (h, w) of an NHWC map adds (b, y, x, channel) and the position
    inside a 16 x 32 output tile of the direct convolution kernels."""
    s = f"row {r} (%256 = {r % 256}) col {c} (%256 = {c % 256})"
    if hw is not None:
        h, w = hw
        y, x = (r // w) % h, r % w
        s += f" = (b {r // (h * w)}, y {y}, x {x}, ch {c}) y%16 = {y % 16} x%32 = {x % 32}"
    return s


def assert_equal_elementwise(out: torch.Tensor, ref: torch.Tensor, what: str, max_report: int = 8, hw=None):
    """`out` must equal `ref` element for element (ref is cast to out's dtype first: one round to nearest even when it is the
    float64 result).  On failure: how many elements differ and the first few as (row, column, got, expected) with
    row % 256 / column % 256, so the tile position is readable.  Leading dimensions are folded into the row.  hw = (h, w):
    out is an NHWC map [..., h, w, channels]; the report adds (b, y, x, channel) and y % 16, x % 32."""
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
        lines.append(f"  {_where(r, c, hw)}: got {float(o2[r, c])!r} expected {float(e2[r, c])!r}")
    raise AssertionError(f"{what}: {nbad} of {o2.numel()} elements differ ({rows_bad} rows, {cols_bad} columns touched); first "
                         f"{len(lines)}:\n" + "\n".join(lines))


def assert_within(out: torch.Tensor, ref64: torch.Tensor, bound: torch.Tensor, what: str, max_report: int = 8, hw=None):
    """|out - ref64| <= bound per element (float64 on out's device); same report as assert_equal_elementwise."""
    d = (out.double() - ref64.to(out.device)).abs()
    bnd = bound.to(out.device)
    bad = ~(d <= bnd)
    if not bool(bad.any()):
        return
    cols = out.shape[-1]
    idx = bad.reshape(-1, cols).nonzero()
    o2, r2, d2, b2 = out.reshape(-1, cols), ref64.to(out.device).reshape(-1, cols), d.reshape(-1, cols), bnd.reshape(-1, cols)
    lines = [f"  {_where(r, c, hw)}: got {float(o2[r, c])!r} expected {float(r2[r, c])!r} "
             f"|diff| {float(d2[r, c]):.3e} > bound {float(b2[r, c]):.3e}" for r, c in idx[:max_report].tolist()]
    raise AssertionError(f"{what}: {int(idx.shape[0])} of {out.numel()} elements outside their bound; worst diff / bound = "
                         f"{float((d / bnd.clamp(min=1e-300)).max()):.3f}; first {len(lines)}:\n" + "\n".join(lines))
