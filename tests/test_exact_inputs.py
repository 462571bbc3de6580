"""The exact-input constructions (tests/exact_inputs.py) keep their promises without any kernel, and the checker notices
the three kinds of local error the whole-matrix norms cannot see.  CPU only."""
import math

import pytest
import torch

import exact_inputs as X

DT16 = [torch.bfloat16, torch.float16]
# every (Tq, Tk) tests/test_gpu_attention_exact.py runs (batch and heads cut down: only the token counts matter here)
ATTN_SHAPES = [(1024, 1024, 1, 2), (672, 672, 2, 2), (576, 576, 2, 2), (196, 196, 1, 2), (200, 150, 2, 3), (65, 129, 1, 2),
               (1, 1, 1, 1)]


# ----------------------------------------------------------------------------------------------- integer GEMM
def test_integer_gemm_is_exact_in_fp32_in_any_k_order():
    """Largest K the GPU tests use (3072): a float32 matmul and a K-permuted float32 matmul both equal float64, the result is
    below 2^24 and far inside the fp16 range, and the operands are exact in both 16-bit types."""
    m, n, k = 300, 132, 3072
    a, w, b = X.int_gemm(m, n, k, seed=1)
    ref = X.gemm_ref64(a[0], w[0], b[0])
    assert float(ref.abs().max()) < 2 ** 24 and float(ref.abs().max()) < 65504 / 16
    perm = torch.randperm(k, generator=torch.Generator().manual_seed(2))
    assert torch.equal((a[0] @ w[0].T + b[0]).double(), ref)
    assert torch.equal((a[0][:, perm] @ w[0][:, perm].T + b[0]).double(), ref)
    # chunked accumulation (a tile's K loop: 64 at a time, partial sums carried in fp32)
    acc = torch.zeros(m, n)
    for k0 in range(0, k, 64):
        acc = acc + a[0][:, k0:k0 + 64] @ w[0][:, k0:k0 + 64].T
    assert torch.equal((acc + b[0]).double(), ref)
    for dt in DT16:
        for t in (a, w, b):
            assert torch.equal(t.to(dt).float(), t)
        r16 = X.randint((m, n), -64, 64, seed=3)
        assert torch.equal(r16.to(dt).float(), r16)
    # the worst case of the ranges, not only this draw: K * 3 * 3 + 64 + 2^20 < 2^24
    assert 3072 * 9 + 64 + 2 ** 20 < 2 ** 24


def test_fold_statistics_and_hi_lo_values_are_exact():
    """Stream integers in [-15, 15], C <= 1024: float32 sums and sums of squares equal float64 in any order; multiples of 1/8
    below 2^15 reconstruct exactly from fp16 hi + fp16 lo."""
    x = X.randint((64, 1024), -15, 15, seed=4)
    st = X.slot_sums64(x, 16)
    assert st.shape == (16, 64, 2)
    assert torch.equal(x.sum(1).double(), st[..., 0].sum(0)) and torch.equal((x * x).sum(1).double(), st[..., 1].sum(0))
    assert torch.equal((x * x).flip(1).sum(1).double(), st[..., 1].sum(0))
    assert 1024 * 225 < 2 ** 24
    assert torch.equal(st.float().double(), st)
    v = X.hilo_values((256, 512), seed=5)
    assert 2 ** 14 < float(v.abs().max()) < 2 ** 15
    hi = v.half()
    lo = (v - hi.float()).half()
    assert torch.equal(hi.float() + lo.float(), v)
    # and the sum of two such values (an EPI_F32_ACCUM update that stays below 2^15) is again one
    v2 = X.hilo_values((256, 512), seed=6, lim=2.0 ** 14) + X.hilo_values((256, 512), seed=7, lim=2.0 ** 14)
    h2 = v2.half()
    assert torch.equal(h2.float() + (v2 - h2.float()).half().float(), v2)


# ------------------------------------------------------------------------------------------ non-linear epilogues
def test_gelu_problem_is_exact_and_covers_the_clamp_region():
    a, w, b = X.gelu_problem(300, 132, seed=11)
    for dt in DT16:
        assert torch.equal(a.to(dt).float(), a) and torch.equal(w.to(dt).float(), w)
    z64 = X.gemm_ref64(a, w, b)
    assert torch.equal((a @ w.T + b).double(), z64)                        # exact in fp32
    assert torch.equal((a.flip(1) @ w.flip(1).T + b).double(), z64)
    frac = float((z64.abs() <= 3).double().mean())
    print(f"gelu z: min {float(z64.min())} max {float(z64.max())} mass in [-3, 3] {frac:.3f}")
    assert frac > 0.5 and float(z64.min()) <= -6 and float(z64.max()) >= 6
    # the kernel clamps erf's argument z / sqrt(2) at +-3: |z| > 4.243 must occur on both sides
    assert int((z64 > 4.5).sum()) > 10 and int((z64 < -4.5).sum()) > 10
    assert len(torch.unique(z64)) > 2000                                    # not a handful of lattice points


def test_rope_trig_error_is_measured_on_the_reference_side():
    e = X.rope_trig_error(64)
    print(f"E_trig = {e:.3e}")
    assert 1e-8 < e < 1e-4                                                  # a float32 angle up to 63 rad: a few 1e-6, times 4
    # the float64 rotation keeps the pair's norm and leaves the other columns alone
    z = X.gemm_ref64(*X.gelu_problem(128, 192, seed=12))
    pos = torch.stack([torch.arange(64), 63 - torch.arange(64)], -1)
    ref, mag = X.rope_ref64(z, pos, 128, 64, 0.25)
    assert torch.equal(ref[:, 128:], z[:, 128:]) and float(mag[:, 128:].abs().max()) == 0.0
    n0 = z[:, 64:80] ** 2 + z[:, 80:96] ** 2
    n1 = ref[:, 64:80] ** 2 + ref[:, 80:96] ** 2
    assert torch.allclose(n0, n1, rtol=1e-12, atol=1e-12)
    assert torch.equal(ref[0, :32], z[0, :32] * 0.25)                       # token 0: y = 0 rotates nothing, q columns scaled


@pytest.mark.parametrize("c", [768, 1024])
@pytest.mark.parametrize("dt", DT16)
def test_fold_consumer_reference_alone_stays_inside_its_bound(c, dt):
    """The fold's own formula in float32 on the CPU, rounded to the output type, against the float64 reference: inside the
    bound the GPU test applies (if it were not, the operation count behind the bound would be wrong)."""
    p = X.fold_consumer_problem(64, c, 136, seed=c)
    for name in ("x", "wf"):
        assert torch.equal(p[name].half().float(), p[name])
    assert torch.equal((p["x"] @ p["wf"].T).double(), p["x"].double() @ p["wf"].double().T)     # exact accumulator
    assert torch.equal(p["colsum"].double(), p["wf"].double().sum(1))
    assert torch.equal(p["bias"].double(), p["b"].double() + p["w0"].double() @ p["beta"].double())
    ref, rstd, acc_abs, mcs_abs, kappa = X.fold_consumer_ref64(p, 1e-6)
    assert float(kappa.max()) <= 2.0
    assert float(ref.abs().max()) < 65504 / 2
    y = X.fold_consumer_f32(p, 1e-6).to(dt)
    bound = X.fold_consumer_bound(ref, rstd, acc_abs, mcs_abs, dt)
    worst = float(((y.double() - ref).abs() / bound).max())
    print(f"fold consumer reference in fp32: worst |diff| / bound = {worst:.3f}")
    X.assert_within(y, ref, bound, "fp32 emulation of the fold consumer")


# ------------------------------------------------------------------------------------------- routing attention
@pytest.mark.parametrize("placement", X.PLACEMENTS)
@pytest.mark.parametrize("shape", ATTN_SHAPES)
def test_routing_gap_and_float64_softmax(shape, placement):
    tq, tk, b, h = shape
    if placement == "perm" and tq != tk:
        return                                                              # a permutation needs Tq == Tk: nothing to check
    q, k, v, pi = X.routing_problem(tq, tk, b, h, seed=tq + tk, placement=placement)
    for dt in DT16:
        for t in (q, k, v):
            assert torch.equal(t.to(dt).float(), t)
    assert int(v.abs().min()) >= 1 and int(v.abs().max()) <= 8
    gap = X.routing_gap_nats(q, k, pi, 0.125)
    assert gap >= 30.0, gap
    if placement == "first":
        assert int(pi.max()) < 64
    if placement == "perm":
        assert all(torch.equal(pi[i, j].sort().values, torch.arange(tk)) for i in range(b) for j in range(h))
    if placement == "spread" and tq >= 16 and tk > 128:
        nt = (tk + 63) // 64
        assert int(pi[..., 0::7].max()) < 64 and int(pi[..., 2::7].min()) >= (nt - 1) * 64 and bool((pi == tk - 1).any())
        assert int(pi[..., 1::7].min()) >= (nt // 2) * 64 and int(pi[..., 1::7].max()) < (nt // 2) * 64 + 64
    for shift in ((0, 1) if b >= 2 else (0,)):
        exp = X.routing_expected(v, pi, shift)
        o = X.softmax_attention64(q, k, v, 0.125, shift)
        assert float((o - exp.double()).abs().max()) < 1e-9
        for dt in DT16:
            assert torch.equal(o.to(dt), exp.to(dt))
    # prescaled entry point: q carries scale * log2(e), rounded to 16 bits; the gap of the ROUNDED operands stays >= 24 nats
    for dt in DT16:
        qs = (q * X.QK_PRESCALE).to(dt)
        gap_p = X.routing_gap_nats(qs.float(), k, pi, math.log(2.0))
        assert gap_p >= 24.0, (dt, gap_p)
        o = X.softmax_attention64(qs.float(), k, v, math.log(2.0))
        assert torch.equal(o.to(dt), X.routing_expected(v, pi).to(dt))
    assert 1024 * math.exp(-24.0) < 2.0 ** -24                              # the row sum is 1.0f for every Tk <= 1024


def test_batch_items_and_heads_have_their_own_values_and_targets():
    q, k, v, pi = X.routing_problem(200, 150, 2, 3, seed=9)
    assert not torch.equal(v[0], v[1]) and not torch.equal(v[0, :, :64], v[0, :, 64:128])
    assert not torch.equal(pi[0], pi[1]) and not torch.equal(pi[0, 0], pi[0, 1])
    e0, e1 = X.routing_expected(v, pi, 0), X.routing_expected(v, pi, 1)
    assert float((e0 != e1).float().mean()) > 0.8                           # the wrong batch item is a visibly different answer
    assert torch.equal(e1[0, 5, 64:128], v[1, pi[0, 1, 5], 64:128])


@pytest.mark.parametrize("tk", [1, 2, 32, 128, 1024])
def test_uniform_attention_mean_is_exact(tk):
    q, k, v = X.uniform_problem(5, tk, 2, 2, seed=tk)
    exp = X.uniform_expected64(v, 5, 1)
    o = X.softmax_attention64(q, k, v, 0.125, 1)
    assert torch.equal(o, exp)                                              # p = 1 / tk and the sums are exact even in float64
    assert torch.equal(exp.float().double(), exp)                           # ... and in fp32: integer sum times 2^-n


# --------------------------------------------------------------------------------- power-of-two softmax weights
# every (Tq, Tk) of test_power_of_two_softmax_every_rescale_path, batch and heads cut down where only the token counts matter
POW2_SHAPES = [(130, 328, 2, 2), (200, 512, 2, 3), (65, 129, 1, 2), (96, 1024, 1, 2), (7, 64, 2, 1)]
_POW2 = {}


def _pow2(shape, variant):
    """(q, k, v, info, {shift: (s, reference dict)}) of one problem, built once for the tests below."""
    if (shape, variant) not in _POW2:
        tq, tk, b, h = shape
        q, k, v, info = X.pow2_problem(tq, tk, b, h, seed=tq + tk + h, variant=variant)
        per_shift = {sh: (X.pow2_scores(q, k, sh), X.pow2_reference(q, k, v, sh)) for sh in ((0, 1) if b >= 2 else (0,))}
        _POW2[(shape, variant)] = (q, k, v, info, per_shift)
    return _POW2[(shape, variant)]


@pytest.mark.parametrize("variant", X.POW2_VARIANTS)
@pytest.mark.parametrize("shape", POW2_SHAPES, ids=str)
def test_power_of_two_problem_keeps_its_conditions(shape, variant):
    """Conditions 1 - 4 of the construction: integer tables in [-127, 127] whose scores are the prescribed table
    entries; every final log2-weight in [-12, 0] or <= -30; flat rows narrow and at least a quarter of the mixed launch
    narrow; every profile present at every shape that has the key tiles for it, with the tile maxima it promises."""
    tq, tk, b, h = shape
    nt = (tk + 63) // 64
    q, k, v, info, per_shift = _pow2(shape, variant)
    prof, table, cls = info["prof"], info["table"], info["cls"]
    name = {n: i for i, n in enumerate(X.POW2_ALL)}
    # 1. integers in range, exact in both 16-bit types; one-hot keys; q k^T is the prescribed table
    assert torch.equal(q, q.round()) and float(q.abs().max()) <= 127
    for dt in DT16:
        for t in (q, k, v):
            assert torch.equal(t.to(dt).float(), t)
    assert bool(((k == 0) | (k == 1)).all()) and torch.equal(k.view(b, tk, h, 64).sum(-1), torch.ones(b, tk, h))
    assert int(v.abs().min()) >= 1 and int(v.abs().max()) <= 8
    assert torch.equal(cls // 4, (torch.arange(tk) // 64).expand(b, h, tk))
    for sh, (s, r) in per_shift.items():
        want = torch.gather(table, 3, cls.roll(-sh, 0)[:, :, None, :].expand(b, h, tq, tk))
        assert torch.equal(s, want.double())
        # 2. the gap, row by row
        assert bool(r["gap_ok"].all()), f"{int((~r['gap_ok']).sum()) // 64} rows with a log2-weight inside (-30, -12)"
        # 3. narrow rows
        nar = r["narrow"].view(b, tq, h, 64)[..., 0].transpose(1, 2)                     # [b,h,tq]
        assert bool(nar[prof == name["flat"]].all())
        assert bool(nar[prof == name["tail-max"]].all()) and bool(nar[prof == name["ripple"]].all())
        if variant == "mixed":
            assert float(nar.double().mean()) >= 0.25
        # the lone maximum of a tail-max row is key tk - 1
        tm = prof == name["tail-max"]
        assert bool((s.argmax(-1)[tm] == tk - 1).all()) and bool(((s == s.amax(-1, keepdim=True)).sum(-1)[tm] == 1).all())
        # what the profiles promise of the tile maxima, relative to the first tile's
        rel = X.pow2_tile_maxima(s)
        rel = rel - rel[..., :1]
        top, arg = rel.amax(-1), rel.argmax(-1)
        big = (rel >= 60).sum(-1)
        if nt > 1:
            for n, lo, hi in (("jump", 37, 40), ("overflow-l", 102, 105), ("overflow-inf", 137, 140)):
                sel = prof == name[n]
                assert bool(((top[sel] >= lo) & (top[sel] <= hi) & (arg[sel] > 0)).all()), n
            sel = prof == name["keeper"]
            assert bool(((big[sel] == 1) & (arg[sel] > 0) & (arg[sel] < nt - 1) & (top[sel] == 70)).all())
            sel = prof == name["keeper-last"]
            assert bool(((big[sel] == 1) & (arg[sel] == nt - 1) & (top[sel] >= 67)).all())
            sel = prof == name["keeper-twice"]
            assert bool(((big[sel] == 2) & (top[sel] == 135) & (arg[sel] < nt - 1) & (rel[..., 1:3].amax(-1)[sel] == 70)).all())
            sel = prof == name["fall"]
            assert bool((rel[..., 1:].amax(-1)[sel] <= -30).all())
            sel = prof == name["stair"]
            step = rel[..., 1:] - rel[..., :-1]
            assert bool((step[sel][:, :max(nt - 2, 0)] >= 3).all()) and bool((step[sel] >= 0).all())
    # 4. every profile that has the tiles for it occurs, in this very shape
    have = set(torch.unique(prof).tolist())
    pool = X.POW2_ALL if variant == "overflow" else X.POW2_PROFILES
    avail = {name[n] for n in pool if X.POW2_MIN_TILES[n] <= nt}
    if variant == "banded":
        # (row // 32 + head + batch) % P reaches every profile only where there are enough bands, heads and batch items
        reach = {(r32 + hh + bb) % len(X.POW2_PROFILES) for r32 in range((tq + 31) // 32) for hh in range(h) for bb in range(b)}
        avail = {name["flat"]} | {i for i in avail if i in reach}
        assert have == avail, (sorted(have), sorted(avail))
        if shape == (200, 512, 2, 3):
            assert have == set(range(len(X.POW2_PROFILES)))
    else:
        assert have == (avail | {name["flat"]}), (sorted(have), sorted(avail))
        if nt >= 6 and tq >= 11:
            assert have == {name[n] for n in pool}
    if variant == "overflow":
        ov = prof >= len(X.POW2_PROFILES)
        assert not bool(ov[:, 1::2].any()) and not bool(ov[:, :, 64:].any())       # rows < 64 of even heads only


def test_power_of_two_profile_assignments():
    """mixed: every 16-row query tile of a wave holds every profile; banded: 32 consecutive rows share one profile; the full
    batch and head counts of the first GPU shape reach every profile in both."""
    p = len(X.POW2_PROFILES)
    mixed, _ = X.pow2_profile_ids(130, 328, 16, 16, "mixed")
    banded, kpos = X.pow2_profile_ids(130, 328, 16, 16, "banded")
    for r0 in range(0, 128, 16):
        assert len(torch.unique(mixed[3, 5, r0:r0 + 16])) == p                  # 6 key tiles: enough for keeper-twice
    assert set(torch.unique(mixed).tolist()) == set(range(p)) == set(torch.unique(banded).tolist())
    for r0 in range(0, 130, 32):
        assert bool((banded[:, :, r0:r0 + 32] == banded[:, :, r0:r0 + 1]).all())
        assert bool((kpos[:, :, r0:r0 + 32] == kpos[:, :, r0:r0 + 1]).all())
    # a profile without the tiles for it is recorded as flat, never silently kept under its own name
    small, _ = X.pow2_profile_ids(200, 150, 2, 3, "overflow")
    assert set(torch.unique(small).tolist()) == {i for i, n in enumerate(X.POW2_ALL) if X.POW2_MIN_TILES[n] <= 3}


@pytest.mark.parametrize("variant", ["mixed", "overflow"])
@pytest.mark.parametrize("shape", POW2_SHAPES, ids=str)
def test_power_of_two_bound_holds_for_float32_online_softmax(shape, variant):
    """The plain online softmax in float32 on the CPU, one key at a time, forward and in reversed key order: within a QUARTER
    of the allowance t on narrow rows and within t on all rows (before the output rounding), and within the full bound after
    rounding to either 16-bit type.  If it were not, the operation count behind c would be wrong."""
    tq, tk, b, h = shape
    q, k, v, info, per_shift = _pow2(shape, variant)
    for sh, (s, r) in per_shift.items():
        vh = v.view(b, tk, h, 64).transpose(1, 2).roll(-sh, 0)
        t = X.pow2_allowance(r, tk)
        for reverse in (False, True):
            emu = X.pow2_online_softmax_f32(s, vh, reverse).transpose(1, 2).reshape(b, tq, h * 64)
            diff = (emu.double() - r["ref"]).abs()
            unit = 2.0 ** -24 * r["A"]
            nar = r["narrow"]
            worst_n = float((diff / unit)[nar].max())
            worst_o = float((diff / t)[~nar].max()) if bool((~nar).any()) else 0.0
            print(f"{shape} {variant} shift {sh} reversed {reverse}: narrow rows {worst_n:.2f} units of 2^-24 A (c = 8); "
                  f"other rows {worst_o:.4f} of t (c = {tk + 8})")
            assert bool((diff[nar] <= t[nar] / 4).all()) and bool((diff <= t).all())
            for dt in DT16:
                X.assert_within(emu.to(dt), r["ref"], X.pow2_bound(r, tk, dt), f"float32 online softmax, {dt}")


def test_power_of_two_bound_sees_a_tail_key_counted_twice_and_a_forgotten_rescale():
    """Two local errors on the reference side: the clamped copy of key Tk - 1 left unmasked once (every row moves, the tail-max
    rows most), and ONE query row whose accumulator misses the 2^-64 of the range keeper (its first tiles weigh 2^64 too
    much) - the checker names that row."""
    shape = (130, 328, 2, 2)
    tq, tk, b, h = shape
    q, k, v, info, per_shift = _pow2(shape, "mixed")
    s, r = per_shift[0]
    bound = X.pow2_bound(r, tk, torch.bfloat16)
    X.assert_within(r["ref"].bfloat16(), r["ref"], bound, "the reference itself")
    k2, v2 = torch.cat([k, k[:, -1:]], 1), torch.cat([v, v[:, -1:]], 1)
    twice = X.pow2_reference(q, k2, v2)["ref"]
    tm = (info["prof"] == X.POW2_ALL.index("tail-max")).transpose(1, 2)[..., None].expand(b, tq, h, 64).reshape(b, tq, h * 64)
    over = (twice - r["ref"]).abs() > bound
    assert float(over[tm].double().mean()) > 0.9
    with pytest.raises(AssertionError):
        X.assert_within(twice.bfloat16(), r["ref"], bound, "tail key counted twice")
    # keeper row (batch 0, head 0): o of the tiles before the event keeps its scale, l is scaled
    row = int((info["prof"][0, 0] == X.POW2_ALL.index("keeper")).nonzero()[0])
    d = s[0, 0, row] - s[0, 0, row].max()
    w = torch.exp2(d)
    event = int(d.argmax()) // 64
    w_bad = w.clone()
    w_bad[:event * 64] *= 2.0 ** 64
    vh = v.view(b, tk, h, 64)[0, :, 0].double()
    bad = r["ref"].clone()
    bad[0, row, :64] = (w_bad @ vh) / w.sum()
    with pytest.raises(AssertionError, match=rf"row {row} "):
        X.assert_within(bad.bfloat16(), r["ref"], bound, "forgotten rescale")


# ----------------------------------------------------------------------------------------- the checker notices
def _correct_answer(dt):
    a, w, b = X.int_gemm(300, 132, 3072, seed=21)
    ref = X.gemm_ref64(a[0], w[0], b[0])
    return ref, ref.to(dt)


@pytest.mark.parametrize("dt", DT16 + [torch.float32])
def test_checker_fails_on_one_element_moved_by_one_ulp(dt):
    ref, out = _correct_answer(dt)
    X.assert_equal_elementwise(out, ref, "correct answer")
    bad = out.clone()
    bad[299, 131] = X.ulp_step(bad[299, 131].reshape(1))[0]
    assert 0 < float((bad.double() - out.double()).abs().max()) <= float(out[299, 131].abs()) * torch.finfo(dt).eps
    rel = float((bad.double() - ref).norm() / ref.norm())
    base = float((out.double() - ref).norm() / ref.norm())
    assert rel - base < 1e-4                                                # what the whole-matrix norm sees of it: nothing
    with pytest.raises(AssertionError) as e:
        X.assert_equal_elementwise(bad, ref, "one ulp")
    msg = str(e.value)
    assert "1 of 39600 elements differ" in msg and "row 299 (%256 = 43) col 131 (%256 = 131)" in msg


def test_checker_fails_on_two_swapped_rows():
    ref, out = _correct_answer(torch.bfloat16)
    bad = out.clone()
    bad[[256, 257]] = out[[257, 256]]
    with pytest.raises(AssertionError) as e:
        X.assert_equal_elementwise(bad, ref, "swapped rows")
    msg = str(e.value)
    assert "(2 rows," in msg and "row 256 (%256 = 0)" in msg


def test_checker_fails_on_a_neighbours_value_row():
    """Attention that reads key j + 1's V row for one key: exactly the rows that target j are wrong."""
    q, k, v, pi = X.routing_problem(200, 150, 2, 3, seed=5)
    exp = X.routing_expected(v, pi)
    X.assert_equal_elementwise(X.softmax_attention64(q, k, v, 0.125).bfloat16(), exp, "float64 softmax")
    j = int(pi[1, 2, 17])
    vbad = v.clone()
    vbad[1, j, 128:192] = v[1, (j + 1) % 150, 128:192]
    got = X.softmax_attention64(q, k, vbad, 0.125).bfloat16()
    hit = int((pi[1, 2] == j).sum())
    with pytest.raises(AssertionError) as e:
        X.assert_equal_elementwise(got, exp, "neighbour's V row")
    assert f"({hit} rows," in str(e.value)
    assert torch.equal(got[0], exp[0].bfloat16())                           # and nothing else moved
    with pytest.raises(AssertionError):                                     # a reference of another shape is refused, not broadcast
        X.assert_equal_elementwise(got[:, :10], exp, "shape")


def test_within_checker_reports_position():
    ref = torch.zeros(300, 132, dtype=torch.float64)
    out = torch.zeros(300, 132)
    out[299, 4] = 1e-3
    X.assert_within(out, ref, torch.full_like(ref, 1.001e-3), "inside the bound")
    with pytest.raises(AssertionError, match=r"row 299 \(%256 = 43\) col 4"):
        X.assert_within(out, ref, torch.full_like(ref, 9e-4), "over the bound")
    out[0, 0] = float("nan")
    with pytest.raises(AssertionError, match="row 0"):
        X.assert_within(out, ref, torch.full_like(ref, 1.0), "nan")


# ------------------------------------------------------------------------------------------ integer convolution
def _conv2d64(x, w, bias, stride, relu_input=False):
    """torch's own float64 convolution of NHWC x [b,h,w,c] with w [cout,3,3,cin]."""
    import torch.nn.functional as F
    xx = x.double().clamp(min=0) if relu_input else x.double()
    y = F.conv2d(xx.permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), None if bias is None else bias.double(), stride=stride, padding=1)
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("shape_stride", [((2, 15, 17, 64, 68), 1), ((1, 15, 17, 64, 68), 2), ((1, 20, 28, 64, 36), 2), ((1, 1, 1, 64, 4), 1)], ids=str)
def test_shifted_slice_reference_equals_conv2d_in_float64(shape_stride):
    (b, h, w, cin, cout), s = shape_stride
    x, wt, bias = X.int_conv(b, h, w, cin, cout, seed=5, groups=2)
    for dt in DT16:
        for t in (x, wt, bias):
            assert torch.equal(t.to(dt).float(), t)
    assert bool((x == 0).any()) and bool(torch.signbit(x[x == 0]).any())        # a few -0.0 are there
    assert not torch.equal(wt[0], wt[1]) and not torch.equal(bias[0], bias[1])
    res = X.randint((2, b) + X.conv_out_size(h, w, s) + (cout,), -64, 64, seed=6)
    for relu_in in (False, True):
        ref = X.conv_ref64(x, wt, bias, res, s, relu_in)
        for g in range(2):
            assert torch.equal(ref[g], _conv2d64(x[g], wt[g], bias[g], s, relu_in) + res[g].double())
    # float32 slices + float32 matmul give the same numbers (the reference of the largest GPU case is built that way)
    assert torch.equal(X.conv_ref64(x, wt, bias, res, s, dtype=torch.float32).double(), X.conv_ref64(x, wt, bias, res, s))


def test_integer_convolution_partial_sums_stay_below_2_24():
    """Largest Cin of the GPU tests (256): the sum of |x| |w| over the window + |bias| + 64 bounds every partial sum any
    order can form - per tap, per 64-channel slice, per split-K plane; worst case of the ranges and this draw in float64."""
    assert 9 * 256 * 9 + 128 < 2 ** 24 and 9 * 256 * 9 + 128 < 65504            # ... and the result is inside the fp16 range
    x, wt, bias = X.int_conv(2, 16, 16, 256, 256, seed=8)
    m = X.conv_max_partial_sum(x, wt, bias)
    assert m <= 9 * 256 * 9 + 128 and m < 2 ** 24
    ref = X.conv_ref64(x, wt, bias)
    cols, wf = X.conv_cols(x), wt.reshape(1, 256, 9 * 256)
    acc = torch.zeros(1, 512, 256)
    for k0 in torch.randperm(36, generator=torch.Generator().manual_seed(1)).tolist():      # K tiles of 64 in a shuffled order, fp32
        acc = acc + cols[..., k0 * 64:(k0 + 1) * 64] @ wf[..., k0 * 64:(k0 + 1) * 64].transpose(-1, -2)
    assert torch.equal((acc + bias[:, None]).double().view(ref.shape), ref)
    with pytest.raises(AssertionError):
        X.int_conv(1, 4, 4, 512, 8, seed=1)


def test_tap_identity_output_is_a_sum_of_nine_known_channels():
    cin, cout = 64, 36
    w = X.tap_identity_weights(cout, cin)
    assert float(w.sum()) == cout * 9 and bool((w.sum(-1) == 1).all())
    x, _, _ = X.int_conv(1, 6, 7, cin, cout, seed=2)
    ref = X.conv_ref64(x[0], w)
    xp = torch.nn.functional.pad(x[0].double(), (0, 0, 1, 1, 1, 1))
    for co in (0, 5, 35):
        want = sum(xp[:, ky:ky + 6, kx:kx + 7, (co + 7 * (3 * ky + kx)) % cin] for ky in range(3) for kx in range(3))
        assert torch.equal(ref[..., co], want)
    w1 = X.tap_identity_weights(128, 128, single_tap=True)
    assert float(w1.sum()) == 128 and bool((w1.flatten(1).sum(1) == 1).all())
    m = torch.randn(2, 6, 8, 128, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    assert torch.equal(X.single_tap_gather(m, 128), X.conv_ref64(m, w1))


@pytest.mark.parametrize("dt", DT16)
def test_conv_checker_names_a_moved_element_and_swapped_taps(dt):
    """One output element moved by one ulp, and two taps of the weights swapped: the checker fails and names the position as
    (b, y, x, channel) with y % 16 and x % 32.  Swapped taps (0, 0) <-> (0, 1) change every row but y = 0 (where both read
    padding), the border column x = 0 included (where one of them does)."""
    b, h, w, cin, cout = 2, 18, 40, 64, 36
    x, wt, bias = X.int_conv(b, h, w, cin, cout, seed=12)
    ref = X.conv_ref64(x[0], wt[0], bias[0])
    out = ref.to(dt)
    X.assert_equal_elementwise(out, ref, "correct answer", hw=(h, w))
    bad = out.clone()
    bad[1, 17, 33, 35] = X.ulp_step(bad[1, 17, 33, 35].reshape(1))[0]
    rel = float((bad.double() - ref).norm() / ref.norm()) - float((out.double() - ref).norm() / ref.norm())
    assert rel < 1e-4                                                       # invisible to the whole-tensor norm
    with pytest.raises(AssertionError) as e:
        X.assert_equal_elementwise(bad, ref, "one ulp", hw=(h, w))
    msg = str(e.value)
    assert f"1 of {b * h * w * cout} elements differ" in msg and "(b 1, y 17, x 33, ch 35) y%16 = 1 x%32 = 1" in msg, msg
    ws = wt[0].clone()
    ws[:, 0, 0], ws[:, 0, 1] = wt[0][:, 0, 1], wt[0][:, 0, 0]
    got = X.conv_ref64(x[0], ws, bias[0]).to(dt)
    with pytest.raises(AssertionError, match=r"\(b 0, y 1, x 0, ch 0\) y%16 = 1 x%32 = 0") as e:
        X.assert_equal_elementwise(got, ref, "swapped taps", hw=(h, w), max_report=4)
    assert f"({b * (h - 1) * w} rows," in str(e.value)
    # a border row that clamps where it should read zero padding: only rows y = 0 differ, and the report says so
    xc = torch.cat([x[0][:, :1], x[0]], 1)                                  # row -1 := row 0
    clamp = X.conv_ref64(xc, wt[0], bias[0])[:, 1:]
    clamp[:, -1] = ref[:, -1]                                               # (the appended row changed the last row's padding too)
    with pytest.raises(AssertionError) as e:
        X.assert_equal_elementwise(clamp.to(dt), ref, "clamped top border", hw=(h, w), max_report=10 ** 6)
    assert " y 0," in str(e.value) and not any(f" y {k}," in str(e.value) for k in range(1, h))


# ----------------------------------------------------------------------------------------------- fused head tail
HEAD4_CASES = [(1, 50, 120, 64, 170, 1), (2, 32, 48, 128, 80, 2), (1, 16, 16, 128, 32, 2), (1, 48, 80, 128, 128, 2)]     # as the GPU tests build them


@pytest.mark.parametrize("case", HEAD4_CASES, ids=str)
def test_head4_problem_is_exact_and_its_bound_holds_for_float32(case):
    """r = (xyz, logit) is exact in fp32 in any order, |xyz| spreads over (0, 6] with exact zeros, the logit over [-8, 8]; the
    float32 evaluation of the kernels' formula, operation by operation, stays inside head4_bounds on its own."""
    b, h, w, cin, seed, groups = case
    p = X.head4_problem(b, h, w, cin, seed, groups)
    for dt in DT16:
        for k in ("x", "w", "w4"):
            assert torch.equal(p[k].to(dt).float(), p[k])
    hmap = torch.relu(X.conv_ref64(p["x"], p["w"], p["bias"]))
    assert float(hmap.max()) <= 10 and torch.equal(hmap, hmap.round())
    r64 = X.head4_r64(p)
    assert torch.equal(r64.float().double(), r64) and torch.equal(r64 * 128, (r64 * 128).round())
    # the projection in float32, in two other orders (channel halves first; reversed)
    hf, w4f = hmap.float(), p["w4"][:, None, None]
    r_a = (hf[..., :64] @ w4f[..., :64].transpose(-1, -2) + hf[..., 64:] @ w4f[..., 64:].transpose(-1, -2)) + p["b4"][:, None, None, None]
    r_b = hf.flip(-1) @ w4f.flip(-1).transpose(-1, -2) + p["b4"][:, None, None, None]
    assert torch.equal(r_a.double(), r64) and torch.equal(r_b.double(), r64)
    assert 128 * 10 * 8 * 2 < 2 ** 24                                       # in units of 2^-7: 14 bits
    d = r64[..., :3].norm(dim=-1)
    zeros = int((d == 0).sum())
    print(f"|xyz|: max {float(d.max()):.3f} zeros {zeros} median {float(d.median()):.3f}; logit in [{float(r64[..., 3].min())}, {float(r64[..., 3].max())}]")
    assert zeros >= 9 * groups * b and float(d.max()) <= 6.0 and float(d.max()) > 3.0 and float(d[d > 0].min()) < 0.25
    assert float(r64[..., 3].abs().max()) <= 8.0 and float(r64[..., 3].max()) > 2.0 and float(r64[..., 3].min()) < -2.0
    e1, e2 = X.exp_f32_errors(r64)
    print(f"E_expm1 = {e1:.3e} E_exp = {e2:.3e} (4 x float32 numpy against float64)")
    assert 2.0 ** -24 < e1 < 2e-6 and 2.0 ** -24 < e2 < 2e-6
    bp, bc = X.head4_bounds(r64, e1, e2)
    assert float(bp[d == 0].abs().max()) == 0.0                             # the clamp branch: pts must be exactly 0
    rp, rc = X.head4_expected64(r64)
    pts, conf = X.head4_f32(r64)
    worst = float(((pts.double() - rp).abs() / bp.clamp(min=1e-300)).max()), float(((conf.double() - rc).abs() / bc).max())
    print(f"float32 formula: worst |diff| / bound = {worst[0]:.3f} (pts) {worst[1]:.3f} (conf)")
    X.assert_within(pts, rp, bp, "float32 tail, pts", hw=(h, w))
    X.assert_within(conf.unsqueeze(-1), rc.unsqueeze(-1), bc.unsqueeze(-1), "float32 tail, conf", hw=(h, w))
    # the bound notices xyz scaled by the neighbouring pixel's norm, and a logit one grid step (2^-7) off
    pb = pts.clone()
    pb[:, :, :, 1:] = pts[:, :, :, 1:] / rp[:, :, :, 1:].norm(dim=-1, keepdim=True).clamp(min=1e-3) * rp[:, :, :, :-1].norm(dim=-1, keepdim=True)
    with pytest.raises(AssertionError):
        X.assert_within(pb, rp, bp, "neighbour's norm", hw=(h, w))
    with pytest.raises(AssertionError):
        X.assert_within((1 + torch.exp(r64[..., 3] + 2.0 ** -7)).float().unsqueeze(-1), rc.unsqueeze(-1), bc.unsqueeze(-1), "logit off", hw=(h, w))


# ------------------------------------------------------------------------------------ x2 align-corners upsample
UP_IN_SIZES = sorted({n // 2 for n in (32, 48, 16, 80, 64)} | {11, 1, 5, 8})      # every input extent the GPU tests upsample


def _fma32(a, b, c):
    """float32 fma(a, b, c) through float64 (a b is exact there; the sum is rounded to float64 first: 2^-53, irrelevant here)."""
    import numpy as np
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def test_constant_map_survives_every_blend_weight_that_occurs():
    """(a): for every float32 weight the kernels compute at the sizes the GPU tests use and every v in [-3, 3], the formula
    a (1 - w) + b w with a = b = v - both blends, with and without FMA contraction - stays within 4 fp32 ulps of v, 2^7
    times closer than the nearest 16-bit rounding midpoint, so the upsampled map is v bit for bit in bf16 and fp16."""
    import numpy as np
    v = np.arange(-3, 4, dtype=np.float32)[:, None, None]
    worst = 0.0
    for n in UP_IN_SIZES:
        _, _, w = X.upsample_coords_f32(n, 2 * n)
        assert w.dtype == np.float32 and float(w.min()) >= 0.0 and float(w.max()) < 1.0
        wx, wy = w[None, :, None], w[None, None, :]
        one = np.float32(1)
        for contract in (False, True):
            if contract:
                blend = lambda a, b, ww: _fma32(b, ww, (a * (one - ww)).astype(np.float32))
            else:
                blend = X.blend_f32
            row = blend(v, v, wx)
            out = blend(row, row, wy)
            worst = max(worst, float(np.abs(out.astype(np.float64) - v).max() / 3.0))
            for dt in DT16:
                assert torch.equal(torch.from_numpy(out).to(dt).float(), torch.from_numpy(np.broadcast_to(v, out.shape).copy()))
    print(f"constant map through both blends: worst relative error {worst:.3e} = {worst / 2.0 ** -23:.2f} ulp")
    assert worst <= 4 * 2.0 ** -23 and worst * 2 ** 7 < 2.0 ** -12 / 2


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("bhw", [(2, 16, 24), (1, 8, 8), (1, 24, 40), (1, 32, 32), (1, 16, 8), (1, 8, 16), (3, 11, 16), (1, 1, 5)], ids=str)
def test_upsample_bound_holds_for_the_float32_formula_and_sees_a_neighbour(bhw, dt):
    """(b): the kernels' formula in float32 on the CPU (float32 coordinates, three blends), rounded to 16 bits, stays inside
    u (|ref| + t) + t of the float64 interpolation with the exact weights - and the same map shifted by ONE source pixel (a
    patch origin off by one) or with the far edge clamped one pixel early leaves it on most elements; the bound is far below
    the difference a neighbouring source pixel makes (ratio printed and asserted)."""
    b, h, w = bhw
    x = X.quarter_values((b, h, w, 16), seed=h * w)
    assert torch.equal(x.to(dt).float(), x) and float(x.abs().max()) <= 4.0
    ref, t = X.upsample2x_ref64(x)
    bound = X.upsample_bound(ref, t, dt)
    y32 = X.upsample2x_f32(x)
    worst = float(((y32.double() - ref).abs() / t.clamp(min=1e-300)).max())
    print(f"float32 formula against float64: worst |diff| / t = {worst:.3f}")
    assert bool(((y32.double() - ref).abs() <= t).all())
    X.assert_within(y32.to(dt), ref, bound, "float32 upsample, rounded", hw=(2 * h, 2 * w))
    if w > 1:
        shifted, _ = X.upsample2x_ref64(x.roll(1, 2))                       # every read one source column to the left
        diff = (shifted - ref).abs()
        seen = float((diff > bound).double().mean())
        ratio = float((diff / bound).median())
        print(f"one source pixel off: {seen:.3f} of the elements leave the bound; median difference / bound = {ratio:.1f}")
        assert seen > 0.9 and ratio > (50 if dt == torch.bfloat16 else 400)
        with pytest.raises(AssertionError):
            X.assert_within(shifted.to(dt), ref, bound, "patch origin off by one", hw=(2 * h, 2 * w))
        if w > 2:
            early = x.clone()
            early[:, :, -1] = x[:, :, -2]                                   # min(.., IW - 2) where min(.., IW - 1) belongs
            with pytest.raises(AssertionError, match=rf"x {2 * w - 1}, ch"):
                X.assert_within(X.upsample2x_ref64(early)[0].to(dt), ref, bound, "far-edge clamp", hw=(2 * h, 2 * w), max_report=10 ** 6)


def test_upsample_reference_equals_interpolate_in_float64():
    import torch.nn.functional as F
    x = X.quarter_values((2, 11, 16, 8), seed=3)
    ref, _ = X.upsample2x_ref64(x)
    want = F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    assert float((ref - want).abs().max()) < 1e-13
    crop, _ = X.upsample2x_ref64(x, 21, 31)
    assert torch.equal(crop, ref[:, :21, :31])
    v, c = X.const_map(2, 4, 6, 8, seed=1, groups=2)
    assert not torch.equal(v[0], v[1]) and not torch.equal(v[0, 0], v[0, 1]) and torch.equal(c[1, 1, 3, 5], v[1, 1])
    assert torch.equal(X.upsample2x_ref64(c)[0], v[:, :, None, None, :].expand(2, 2, 8, 12, 8).double())


# ----------------------------------------------------------------------------------------- host-level contracts
def test_rope_bound_checks_its_promise():
    """ops.rope_bound verifies 0 <= pos and pos < bound once, on the host, before any launch relies on the promise."""
    from mast3r_slam import ops
    ok = torch.stack([torch.arange(12), torch.arange(12).flip(0)], -1).to(torch.int32)
    assert ops.rope_bound(ok, 12) is ok and ops._rope_pmax(ok) == 12
    neg = ok.clone()
    neg[3, 1] = -1
    with pytest.raises(ValueError, match="negative"):
        ops.rope_bound(neg, 12)
    high = ok.clone()
    with pytest.raises(ValueError, match="bound"):
        ops.rope_bound(high, 11)
    assert ops._rope_pmax(neg) == 0 and ops._rope_pmax(high) == 0           # a refused promise is not recorded
    with pytest.raises(ValueError):
        ops.rope_bound(ok.long(), 12)
    with pytest.raises(ValueError):
        ops.rope_bound(ok, 0)
