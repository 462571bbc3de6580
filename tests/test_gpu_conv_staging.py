"""Weight and patch staging of the direct convolution kernel (conv_tail.hip) through its three entry points
m3_conv3x3_direct_grouped2_dt, m3_conv3x3_up_direct_grouped2_dt and m3_dpt_tail_grouped2_dt.  A workgroup stages the weights
of a (tap, 64-channel slice) step from ITS weight rows - the group's tensor (blockIdx.y), the output-channel half (blockIdx.z,
Cout = 256) - and, with the fused x2 upsample, an input patch whose origin moves with the tile.  So: one and two groups,
Cin and Cout 128 / 256 (2 or 4 slices, one or two halves), maps of 16 x 16 (the tile's right half outside), 16 x 48 and
32 x 32 (a second tile row), a 64 x 64 output upsampled from 32 x 32 (tiles with px0, py0 > 0 and all four corners) - and
weights and input passed as views into larger allocations whose other rows hold a sentinel: a wrong base reads it.

Expected values and bounds are those of tests/exact_inputs.py: integer convolutions bit for bit against float64, the head
tail and the upsample's blend per element with the bounds defined there."""
import contextlib

import pytest
import torch

import exact_inputs as X
from mast3r_slam import ops

pytestmark = pytest.mark.gpu

DT16 = [torch.bfloat16, torch.float16]
SIZES = [(16, 16), (16, 48), (32, 32)]
SENTINEL = 512.0                                  # exact in both 16-bit types
GUARD_BEFORE, GUARD_AFTER = 37, 5                 # rows (pixels / output channels) around an operand


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


def guarded(t: torch.Tensor, dt, dev, row_dims: int = 1):
    """t (CPU float32) as a contiguous view of dtype dt into an allocation with 37 sentinel rows before and 5 after; a row
    is the last `row_dims` dimensions (a pixel's channels; an output channel's [3, 3, Cin] weights)."""
    inner = 1
    for d in t.shape[-row_dims:]:
        inner *= d
    rows = t.reshape(-1, inner)
    r = rows.shape[0]
    big = torch.full((GUARD_BEFORE + r + GUARD_AFTER, inner), SENTINEL, dtype=dt, device=dev)
    big[GUARD_BEFORE:GUARD_BEFORE + r] = rows.to(dt).to(dev)
    view = big[GUARD_BEFORE:GUARD_BEFORE + r].view(t.shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return view


def _sq(t, groups):
    return t if groups == 2 else t[0]


def _operands(x, wt, dt, dev, groups):
    """x [g,b,h,w,cin] as ONE guarded view (the groups back to back), each group's weights as its own guarded view."""
    return _sq(guarded(x, dt, dev), groups), [guarded(wt[g], dt, dev, row_dims=3) for g in range(groups)]


# ----------------------------------------------------------------------- m3_conv3x3_direct_grouped2_dt
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("dt", DT16, ids=_name)
@pytest.mark.parametrize("cout", [128, 256])
@pytest.mark.parametrize("cin", [128, 256])
def test_direct_conv_weight_rows_bit_exact(dev, cin, cout, dt, groups):
    """conv3x3(direct=True) on integer operands: plain output on every size, the residual-add and the relu epilogue (their own
    instantiations) on the two-row map."""
    fails = Failures()
    for i, (h, w) in enumerate(SIZES):
        x, wt, bias = X.int_conv(1, h, w, cin, cout, seed=300 + i + cin + cout + groups, groups=groups)
        xv, wv = _operands(x, wt, dt, dev, groups)
        bd = bias.to(dev)
        ref = X.conv_ref64(x.to(dev), wt.to(dev), bd)
        epis = [("bf16", ops.EPI_BF16)] + ([("bf16_add", ops.EPI_BF16_ADD), ("bf16_relu", ops.EPI_BF16_RELU)] if (h, w) == (32, 32) else [])
        for epi_name, epi in epis:
            with fails.case():
                resid = rd = None
                if epi == ops.EPI_BF16_ADD:
                    rd = X.randint((groups, 1, h, w, cout), -64, 64, seed=i).to(dt).to(dev)
                    resid = _sq(rd, groups).contiguous()
                if groups == 2:
                    got = ops.conv3x3_grouped2(xv, wv[0], wv[1], bd[0], bd[1], epi, resid=resid, direct=True)
                else:
                    got = ops.conv3x3(xv, wv[0], bd[0], epi, resid=resid, direct=True)
                exp = ref if rd is None else ref + rd.double()
                exp = torch.relu(exp) if epi == ops.EPI_BF16_RELU else exp
                X.assert_equal_elementwise(got, _sq(exp, groups), f"direct conv {epi_name} {_name(dt)} {h}x{w} {cin}->{cout} groups={groups}",
                                           hw=(h, w))
    fails.done()


# -------------------------------------------------------------------- m3_conv3x3_up_direct_grouped2_dt
def _up_direct(xv, wv, bd, upsample, groups):
    if groups == 2:
        return ops.conv3x3_up_direct_grouped2(xv, wv[0], wv[1], bd[0], bd[1], upsample=upsample)
    return ops.conv3x3_up_direct(xv, wv[0], bd[0], upsample=upsample)


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("dt", DT16, ids=_name)
@pytest.mark.parametrize("cin", [128, 256])
def test_up_direct_without_upsample_bit_exact(dev, cin, dt, groups):
    fails = Failures()
    for i, (h, w) in enumerate(SIZES):
        with fails.case():
            x, wt, bias = X.int_conv(1, h, w, cin, 128, seed=400 + i + cin + groups, groups=groups)
            xv, wv = _operands(x, wt, dt, dev, groups)
            bd = bias.to(dev)
            got = _up_direct(xv, wv, bd, False, groups)
            X.assert_equal_elementwise(got, _sq(X.conv_ref64(x.to(dev), wt.to(dev), bd), groups),
                                       f"up_direct plain {_name(dt)} {h}x{w} cin={cin} groups={groups}", hw=(h, w))
    fails.done()


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("dt", DT16, ids=_name)
@pytest.mark.parametrize("cin", [128, 256])
def test_up_direct_upsampled_64x64(dev, cin, dt, groups):
    """64 x 64 from 32 x 32.  (a) a map constant per channel: every blend returns the constant, the output is the integer
    convolution at the upsampled resolution, bit for bit.  (b) multiples of 1/4 under one tap of weight 1 per output channel:
    each output is ONE interpolated value, bound exact_inputs.upsample_bound - a patch origin off by one shows at its seam."""
    h = w = 64
    fails = Failures()
    with fails.case():
        v, x = X.const_map(1, h // 2, w // 2, cin, seed=500 + cin, groups=groups)
        _, wt, bias = X.int_conv(1, 1, 1, cin, 128, seed=510 + cin, groups=groups)
        xv, wv = _operands(x, wt, dt, dev, groups)
        bd = bias.to(dev)
        got = _up_direct(xv, wv, bd, True, groups)
        up = v.to(dev)[:, :, None, None, :].expand(groups, 1, h, w, cin)
        X.assert_equal_elementwise(got, _sq(X.conv_ref64(up, wt.to(dev), bd), groups),
                                   f"up_direct constant {_name(dt)} cin={cin} groups={groups}", hw=(h, w))
    with fails.case():
        x = X.quarter_values((groups, 1, h // 2, w // 2, cin), seed=520 + cin)
        w0 = X.tap_identity_weights(128, cin, single_tap=True)
        wt = torch.stack([w0.roll(5 * g, 0) for g in range(groups)])
        xv, wv = _operands(x, wt, dt, dev, groups)
        got = _up_direct(xv, wv, [None, None], True, groups)
        up, t = X.upsample2x_ref64(x)
        ref = torch.stack([X.single_tap_gather(up[g], 128).roll(5 * g, -1) for g in range(groups)])
        tt = torch.stack([X.single_tap_gather(t[g], 128).roll(5 * g, -1) for g in range(groups)])
        X.assert_within(got.cpu(), _sq(ref, groups), _sq(X.upsample_bound(ref, tt, dt), groups),
                        f"up_direct position {_name(dt)} cin={cin} groups={groups}", hw=(h, w))
    fails.done()


# ------------------------------------------------------------------------------ m3_dpt_tail_grouped2_dt
def _check_tail(pts, conf, r64, what, hw):
    e1, e2 = X.exp_f32_errors(r64)
    print(f"{what}: E_expm1 = {e1:.3e} E_exp = {e2:.3e}")
    bp, bc = X.head4_bounds(r64, e1, e2)
    rp, rc = X.head4_expected64(r64)
    X.assert_within(pts.cpu(), rp, bp, what + " pts", hw=hw)
    X.assert_within(conf.cpu().unsqueeze(-1), rc.unsqueeze(-1), bc.unsqueeze(-1), what + " conf", hw=hw)


def _dpt_tail(p, xv, wv, dt, dev, groups, upsample):
    w4, b4, bias = p["w4"].to(dt).to(dev), p["b4"].to(dev), p["bias"].to(dev)
    if groups == 2:
        return ops.dpt_tail_grouped2(xv, wv[0], wv[1], bias[0], bias[1], w4[0], w4[1], b4[0], b4[1], upsample=upsample)
    return ops.dpt_tail(xv, wv[0], bias[0], w4[0], b4[0], upsample=upsample)


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("dt", DT16, ids=_name)
def test_dpt_tail_per_element(dev, dt, groups):
    """The fused tail at an exact r (exact_inputs.head4_problem, bounds head4_bounds): the three sizes without the upsample,
    and 64 x 64 from a 32 x 32 map constant per channel."""
    fails = Failures()
    for h, w in SIZES:
        with fails.case():
            p = X.head4_problem(1, h, w, 128, seed=600 + h + w, groups=groups)
            xv, wv = _operands(p["x"], p["w"], dt, dev, groups)
            pts, conf = _dpt_tail(p, xv, wv, dt, dev, groups, False)
            _check_tail(pts, conf, _sq(X.head4_r64(p), groups), f"dpt_tail {_name(dt)} {h}x{w} groups={groups}", (h, w))
    with fails.case():
        h = w = 64
        p = X.head4_problem(1, 4, 4, 128, seed=610, groups=groups)
        v, x = X.const_map(1, h // 2, w // 2, 128, seed=620, groups=groups)
        xv, wv = _operands(x, p["w"], dt, dev, groups)
        pts, conf = _dpt_tail(p, xv, wv, dt, dev, groups, True)
        r64 = _sq(X.head4_r64(p, x=v[:, :, None, None, :].expand(groups, 1, h, w, 128)), groups)
        _check_tail(pts, conf, r64, f"dpt_tail upsampled constant {_name(dt)} groups={groups}", (h, w))
    fails.done()
