"""CPU: the bound of the token-mixing operators (tests/attn_ref.py) has teeth, and the route
report names the route every row of tests/test_gpu_attn_family.py is meant to take.

SwinBlock and A2_Attn in fp32 with every matrix product as a fp16 two-term split keep
|y - ref64| <= K E32 + 2^-23 |ref64| on every case, NaN and Inf ones included; a split that drops one low-term product
of one matrix product breaks it. The oracles in fp32 and fp64 agree on where the output is NaN, and at most half of any
NaN case's output is NaN, so the rest is still held to the bound."""
import pytest
import torch

import attn_ref as ar
from yolosod_amd import _hip

EMULATED = [ms for ms in ar.MODULE_SHAPES if ms[0] != "MambaBlock"]
# the mutants run where their ratios were measured: two SwinBlock and two A2_Attn shapes
MUTATED = [("SwinBlock", (64, 2, 7), (2, 64, 20, 13)), ("SwinBlock", (256, 4, 7), (1, 256, 14, 9)),
           ("A2_Attn", (192, None, 4, 3), (2, 192, 10, 20)), ("A2_Attn", (64, None, 8, 8), (2, 64, 4, 8))]
# (1, 512, 9, 9): the NaN's window is 49 of 81 pixels (share 0.605); hd 128 meets NaN in the attention piece test
NAN_CASES = [ms for ms in ar.MODULE_SHAPES if ms[2] != (1, 512, 9, 9)]


def _id(ms):
    return f"{ms[0]}-{'-'.join(map(str, ms[1]))}-{'x'.join(map(str, ms[2]))}"


@pytest.mark.parametrize("ms", EMULATED, ids=_id)
def test_emulation_keeps_the_bound(ms):
    op, args, shape = ms
    for kind in ar.INPUTS:
        x, ref = ar.case_data(op, args, shape, kind)
        assert ref.e32 > 0 and bool(torch.isfinite(ref.ref64).all())
        y = ar.emulate(op, args, x, kind == "sharp")
        print(f"family {_id(ms)} {kind}: emulation ratio to E32 {ar.e32_ratio(y, ref.ref64, ref.e32):.3f} "
              f"(E32 {ref.e32:.3g}, max|ref| {float(ref.ref64.abs().max()):.1f})")
        assert ar.worst_ratio(y, ref.ref64, ref.e32) <= 1.0, (ms, kind)


@pytest.mark.parametrize("ms", MUTATED, ids=_id)
def test_every_mutant_breaks_the_bound(ms):
    """On the structured input, plain and sharpened, every one of the mutants exceeds the bound."""
    op, args, shape = ms
    for kind in ("structured", "sharp"):
        x, ref = ar.case_data(op, args, shape, kind)
        for mutant in ar.MUTANTS[op]:
            y = ar.emulate(op, args, x, kind == "sharp", mutant)
            r = ar.worst_ratio(y, ref.ref64, ref.e32)
            print(f"family {_id(ms)} {kind}: {mutant[0]}/{mutant[1]} {ar.e32_ratio(y, ref.ref64, ref.e32):.3g} E32")
            assert r > 1.0, (ms, kind, mutant, r)


@pytest.mark.parametrize("special", ["nan", "inf"])
@pytest.mark.parametrize("ms", NAN_CASES, ids=_id)
def test_nan_cases_leave_half_of_the_output_to_the_bound(ms, special):
    """NaN or +Inf at x[0, 3, 2, 4]: the oracles agree in fp32 and fp64 on the non-finite mask, which is all NaN (an Inf
    meets the LayerNorm, or 0 * Inf in SiLU), at most half of the output, and not empty; the emulation has the same
    mask and keeps the bound elsewhere."""
    op, args, shape = ms
    x, ref = ar.case_data(op, args, shape, "structured", special)
    mask = torch.isnan(ref.ref64)
    assert torch.equal(mask, ref.nonfinite32) and torch.equal(mask, ~torch.isfinite(ref.ref64))
    share = ar.nan_share(ref.ref64)
    print(f"family {_id(ms)} {special}: NaN share {share:.3f}")
    assert 0.0 < share <= 0.5
    assert bool(mask[ar.SPECIAL_AT])
    if op != "MambaBlock":
        y = ar.emulate(op, args, x)
        assert ar.worst_ratio(y, ref.ref64, ref.e32) <= 1.0


def test_structured_inputs_have_the_structure():
    shape = (2, 64, 20, 13)
    x = ar.structured(shape, 3)
    assert torch.equal(x, ar.structured(shape, 3))
    assert float(x[:, 0].mean()) > ar.OFFSET - 1 and abs(float(x[:, 1].mean())) < 1.5       # offset planes
    assert float(x[:, 1::5, 6:9, 4:8].mean()) > ar.OFFSET - 1                                # the 3x4 block, all channels
    assert bool((x[:, :, 0, 0] == ar.OUTLIER).all()) and bool((x[:, :, -1, -1] == -ar.OUTLIER).all())
    assert bool((x[:, :, 13, :] == 0.75).all())                                              # a constant row
    assert not bool(ar.zeros(shape).any())
    assert int(torch.isnan(ar.with_nan(x)).sum()) == 1 and bool(torch.isnan(ar.with_nan(x))[ar.SPECIAL_AT])
    assert int(torch.isinf(ar.with_inf(x)).sum()) == 1 and float(ar.with_inf(x)[ar.SPECIAL_AT]) == float("inf")


def test_sharpen_peaks_the_softmax_rows():
    """Mean of the largest attention probability per row (windows with zero-pad tokens included): diffuse at recipe
    parameters, while a sharpened row gives more than half its mass to one key."""
    op, args, shape = "SwinBlock", (64, 2, 7), (2, 64, 20, 13)
    x = ar.make_input(op, args, shape, "structured")
    peaks = []
    for sharp in (False, True):
        m = ar.build(op, args, sharp)
        wa, at = m.window_attn, m.window_attn.attn
        with torch.inference_mode():
            t = torch.nn.functional.conv2d(x, m.dw.weight, padding=1, groups=64)
            win, _, _ = ar.R.window_partition_ref(t, 7)
            u = torch.nn.functional.layer_norm(win, (64,), wa.norm1.weight, wa.norm1.bias, wa.norm1.eps)
            qkv = u @ at.in_proj_weight.t() + at.in_proj_bias
            q, k = (v.reshape(-1, 49, 2, 32).transpose(1, 2) for v in qkv.split(64, -1)[:2])
            p = torch.softmax(q @ k.transpose(-1, -2) / 32 ** 0.5, -1)
        peaks.append(float(p.amax(-1).mean()))
    assert peaks[0] < 0.4 and peaks[1] > 0.5, peaks


def _set(lib, switches):
    """Apply ((name, value), ...); returns the undo list."""
    undo = []
    for name, v in switches:
        prev = getattr(lib, f"yolosod_debug_set_{name}")(v)
        undo.append((name, 1 if prev is None else prev))  # set_swin_fused returns nothing; its default is 1
    return undo


@pytest.mark.parametrize("row", ar.SWIN_ROWS, ids=lambda r: r.id)
def test_route_report_names_the_intended_route(row):
    lib = _hip.load_library()
    B, C, H, W = row.shape
    undo = _set(lib, row.switches)
    try:
        assert _hip.swin_route(B, C, row.args[1], H, W, row.args[2], 2 * C) == row.route
    finally:
        _set(lib, undo)


def test_route_report_follows_the_launchers_conditions():
    """The bail-outs of the three launchers: hidden != 2C, more than 2^31 windows, an image of 2^30 elements, a shape the
    entry rejects."""
    route = _hip.swin_route
    assert route(1, 64, 2, 14, 14, 7, 128) == "split_fused"
    assert route(1, 64, 2, 14, 14, 7, 256) == "decomposed"          # mlp_hidden != 2C: no fused kernel
    assert route(1, 64, 8, 14, 14, 7, 128) == "decomposed"          # 8 heads: not instantiated
    assert route(1, 64, 2, 4096, 4096, 7, 128) == "decomposed"      # C H W = 2^30: 32-bit byte offsets
    assert route(1 << 20, 64, 2, 320, 320, 7, 128) == "decomposed"  # B nWin >= 2^31: 32-bit window indices
    assert route(1, 256, 4, 7, 6, 7, 512) == "decomposed" and route(1, 256, 4, 7, 7, 7, 512) == "split_fused"
    assert route(1, 128, 4, 7, 6, 7, 256) == "exact_fused"
    with pytest.raises(RuntimeError, match="unsupported"):
        route(1, 48, 2, 14, 14, 7, 96)                              # C % 32 != 0
    with pytest.raises(RuntimeError, match="unsupported"):
        route(1, 64, 2, 19, 19, 19, 128)                            # 361 tokens per window
