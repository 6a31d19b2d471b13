"""CPU: the channel-attention bound (tests/channel_ref.py) has teeth. The fp32 emulation of SE,
CBAM and CA in the kernels' summation order keeps |y - ref64| <= K E32 + 2^-23 |ref64| on every case of
tests/test_gpu_channel_attn.py, and every mutant that loses one thing (a max started from 0, a border map that is not
zero, a dropped last part, a mean over the padded length, a wrong gate for the channel tail, a skipped short group, zero
column means past 256) breaks it on every case that can reach it - so the structured inputs discriminate; a ReLU that
swallows a NaN is shown by the NaN mask. Also: the Python restatement of the plane segmentation equals the library's."""
import ctypes

import pytest
import torch

import channel_ref as cr

ALL = [(op, c) for op, cases in cr.CASES.items() for c in cases]


def _reaches(mutant, op, shape):
    """Whether the mutated thing exists at this case at all."""
    B, C, H, W = shape
    parts, seg = cr.part_plan(H * W)
    pooled = op in ("SE_Block", "CBAM_Block")
    return {"max_init0": op == "CBAM_Block", "pad_neg_inf": op == "CBAM_Block",
            "drop_last_part": pooled and parts > 1, "mean_padded": pooled and parts * seg != H * W,
            "chan_tail": pooled and C % 8 != 0, "group_tail": op == "CBAM_Block" and C > 32 and C % 32 != 0,
            "ca_col_hi": op == "CA_Block" and W > 256}[mutant]


@pytest.mark.parametrize("op,case", ALL, ids=[f"{op}-{cr.case_id(c)}" for op, c in ALL])
def test_emulation_keeps_the_bound_and_mutants_break_it(op, case):
    shape, arg, _ = case
    x, ref64, e32 = cr.case_data(op, shape, arg)
    assert e32 > 0 and bool(torch.isfinite(ref64).all())
    y = cr.emulate(op, arg, x)
    print(f"family {op} {cr.case_id(case)}: emulation ratio to E32 {cr.e32_ratio(y, ref64, e32):.3f} (E32 {e32:.3g})")
    r = cr.worst_ratio(y, ref64, e32)
    assert r <= 1.0, (op, case, r)
    for mutant in cr.MUTANTS[:-1]:
        if not _reaches(mutant, op, shape):
            continue
        rm = cr.worst_ratio(cr.emulate(op, arg, x, mutant), ref64, e32)
        print(f"family {op} {cr.case_id(case)}: {mutant} {rm:.3g}")
        assert rm > 1.0, (op, case, mutant, rm)


def test_every_mutant_is_reached_by_a_case():
    """The test above shows a mutant on every case that reaches it; each one is reached (relu_swallows_nan: below)."""
    for mutant in cr.MUTANTS[:-1]:
        assert any(_reaches(mutant, op, case[0]) for op, case in ALL), mutant


@pytest.mark.parametrize("op", list(cr.CASES))
@pytest.mark.parametrize("shape", cr.NAN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_nan_mask_follows_the_oracle_and_the_laundering_mutant_loses_it(op, shape):
    """One NaN at x[1, 3, 2, 4]: the emulation's NaN mask is the oracle's (the whole image for SE and CBAM, the NaN's row
    and column in every channel for CA) and image 0 keeps its bits; with fmaxf-style maxes and clamps (the kernels'
    behaviour before the fix) the mask shrinks: to the NaN element itself for SE and CA, to the 7x7 window that CBAM's
    spatial conv spreads the pixel's NaN channel sum over."""
    arg = cr.NAN_ARG[op]
    x = cr.structured(shape, 11)
    xn = cr.with_nan(x)
    ref64, _ = cr.oracle(op, arg, xn)
    mask = torch.isnan(ref64)
    assert not bool(mask[0].any())
    if op == "CA_Block":
        want = torch.zeros(shape, dtype=torch.bool)
        want[1, :, cr.NAN_AT[2], :] = True
        want[1, :, :, cr.NAN_AT[3]] = True
        assert torch.equal(mask, want)
    else:
        assert bool(mask[1].all())
    y, yn = cr.emulate(op, arg, x), cr.emulate(op, arg, xn)
    assert torch.equal(torch.isnan(yn), mask)
    assert torch.equal(yn[0], y[0])
    bad = cr.emulate(op, arg, xn, "relu_swallows_nan")
    lost = torch.isnan(bad)
    if op == "CBAM_Block":
        win = torch.zeros(shape, dtype=torch.bool)
        win[1, :, max(cr.NAN_AT[2] - 3, 0):cr.NAN_AT[2] + 4, max(cr.NAN_AT[3] - 3, 0):cr.NAN_AT[3] + 4] = True
        assert torch.equal(lost, win)
    else:
        assert int(lost.sum()) == 1 and bool(lost[cr.NAN_AT])


def test_structured_inputs_have_the_structure():
    shape = (1, 8, 172, 143)
    x = cr.structured(shape, 3)
    assert torch.equal(x, cr.structured(shape, 3))
    parts, seg = cr.part_plan(172 * 143)
    assert (parts, seg) == (3, 8200)
    assert bool((x[:, 2::3] < 0).all())                                  # (a) negative planes
    assert bool((x[:, :, :5, :5] < 0).all()) and float(x.amax(1).min()) < 0  # (b) pixels negative in every channel
    assert float(x[:, 0].mean()) > cr.OFFSET - 1 and float(x[:, 5].mean()) < 0      # (c) offset planes; (a) wins where both hold
    xf = x.view(1, 8, -1)
    for i in (172 * 143 - 1, seg - 1, seg, 2 * seg - 1, 2 * seg):        # (d) outliers on both sides of the boundaries
        assert bool((xf[0, [1, 3, 4, 6, 7], i].abs() == cr.OUTLIER).all()) and bool((xf[0, [2, 5], i] == -cr.OUTLIER).all())


@pytest.mark.parametrize("HW", [1, 5, 8191, 16380, 16383, 16384, 16637, 24596, 65280, 65536, 524288, 600000])
def test_part_plan_equals_the_library(HW):
    from yolosod_amd import _hip
    seg = ctypes.c_long(0)
    parts = _hip.load_library().yolosod_plane_parts(HW, ctypes.byref(seg))
    assert cr.part_plan(HW) == (int(parts), int(seg.value))
    assert (parts - 1) * seg.value < HW <= parts * seg.value and 1 <= parts <= 64
