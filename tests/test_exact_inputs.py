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
