"""CPU: the bounds tests/test_gpu_attn_bf16.py holds the bf16 kernels to (tests/attn_bf16_ref.py, DESIGN.md sections 9
and 33) are reachable with room and have teeth, shown on the reference emulation alone - never on the kernels.

SwinBlock and A2_Attn in fp32 with a round-to-bf16 at every storage point stay inside the block bound on every row and
input kind; every mutant that applies to a row breaks the bound on at least one input kind the GPU test runs for that
row; at most half of a NaN case's output is NaN; the attention piece with P rounded to bf16 keeps the GEMM / attention
bound with q and k sharpened; and the report hooks name the form every row is meant to take."""
import pytest
import torch

import attn_bf16_ref as br
from yolosod_amd import _hip

# the rows whose oracle NaN share exceeds 0.5 (left out of the GPU NaN test): one 7x7 window of 81 pixels (0.605),
# and A2_Attn at B = 1, where the NaN token is a key of the only image (1.0)
NAN_LEFT_OUT = {("SwinBlock", (1, 512, 9, 9)), ("A2_Attn", (1, 128, 12, 40)), ("A2_Attn", (1, 256, 12, 24))}


def _id(ms):
    return f"{ms[0]}-{'-'.join(map(str, ms[1]))}-{'x'.join(map(str, ms[2]))}"


def _row_of(ms):
    return next(r for r in br.ROWS if (r.op, r.args, r.shape) == ms)


@pytest.mark.parametrize("ms", br.MODULE_SHAPES, ids=_id)
def test_emulation_keeps_the_block_bound(ms):
    op, args, shape = ms
    for kind in br.INPUTS:
        x, ref = br.case_data(op, args, shape, kind)
        assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
        mx, mean = br.ratios(br.emulate(op, args, x, kind == "sharp"), ref)
        print(f"bf16 {_id(ms)} {kind}: emulation max {mx:.4f} mean {mean:.4f}")
        assert mx <= br.BLOCK_MAX and mean <= br.BLOCK_MEAN, (ms, kind, mx, mean)


@pytest.mark.parametrize("ms", br.MODULE_SHAPES, ids=_id)
def test_every_applicable_mutant_breaks_the_bound_on_some_input(ms):
    op, args, shape = ms
    row = _row_of(ms)
    for mutant in br.MUTANTS[op]:
        if not br.applies(mutant, row):
            continue
        caught = []
        for kind in br.INPUTS:
            x, ref = br.case_data(op, args, shape, kind)
            mx, mean = br.ratios(br.emulate(op, args, x, kind == "sharp", mutant), ref)
            print(f"bf16 {_id(ms)} {kind}: {mutant} max {mx:.4f} mean {mean:.4f}")
            if mx > br.BLOCK_MAX or mean > br.BLOCK_MEAN:
                caught.append(kind)
        assert caught, (ms, mutant)


def test_every_mutant_applies_to_a_row_of_every_kernel_family():
    """Each mutant is exercised on a fused SwinBlock row and a decomposed one (the left halo and the pad tokens are
    also the token kernels' business), and on an A2_Attn row."""
    fused = [r for r in br.SWIN_ROWS if r.route.startswith("fused")]
    decomposed = [r for r in br.SWIN_ROWS if r.route.startswith("decomposed")]
    for mutant in br.SWIN_MUTANTS:
        assert any(br.applies(mutant, r) for r in fused), mutant
        assert any(br.applies(mutant, r) for r in decomposed), mutant
    for mutant in br.A2_MUTANTS:
        assert any(br.applies(mutant, r) for r in br.A2_ROWS), mutant


@pytest.mark.parametrize("ms", br.MODULE_SHAPES, ids=_id)
def test_nan_share_and_emulated_mask(ms):
    """NaN at x[0, 3, 2, 4]: the oracle's NaN mask is not empty; where its share is at most 0.5 the emulation has the
    same mask and keeps the bound on the rest; the rows above 0.5 are exactly those the GPU test leaves out."""
    op, args, shape = ms
    x, ref = br.case_data(op, args, shape, "structured", True)
    mask = torch.isnan(ref)
    share = float(mask.double().mean())
    print(f"bf16 {_id(ms)} nan: share {share:.3f}")
    assert bool(mask.any()) and torch.equal(mask, ~torch.isfinite(ref))
    assert (share > 0.5) == ((op, shape) in NAN_LEFT_OUT), (ms, share)
    if share <= 0.5:
        y = br.emulate(op, args, x)
        assert torch.equal(torch.isnan(y), mask)
        assert br.within(y, ref), (ms, br.ratios(y, ref))


@pytest.mark.parametrize("L,C,heads", br.ATTN_CASES)
def test_attention_emulation_keeps_the_bound_plain_and_sharpened(L, C, heads):
    for sharp in (False, True):
        qkv = br.attn_qkv(L, C, heads, sharp)
        ref = br.ar.attention_ref(qkv.double(), br.ATTN_NSEQ, L, C, heads)
        d = (br.attention_emul(qkv, br.ATTN_NSEQ, L, C, heads).double() - ref).abs()
        hd = C // heads
        q, k, _ = qkv.double().view(br.ATTN_NSEQ, L, 3, heads, hd).permute(2, 0, 3, 1, 4)
        peak = float(torch.softmax(q @ k.transpose(-1, -2) / hd ** 0.5, -1).amax(-1).mean())
        r = float((d / br.gemm_limit(ref)).max())
        print(f"bf16 attention L={L} C={C} heads={heads} sharp={sharp}: emulation {r:.3f} of the bound, mean peak {peak:.2f}")
        assert r <= 1.0, (L, C, heads, sharp, r)
        if sharp:
            assert peak >= 0.5  # the rows are peaked


def test_report_hooks_name_the_forms_of_the_rows():
    """Host only: the route of every SwinBlock row, the attention form of every row and piece case, the tile of every
    GEMM shape of the GPU file, and the refusals."""
    lib = _hip.load_library()
    for row in br.SWIN_ROWS + br.TILE128_ROWS:
        B, C, H, W = row.shape
        prev = [(n, getattr(lib, f"yolosod_debug_set_{n}")(v)) for n, v in row.switches]
        try:
            assert _hip.swin_bf16_route(B, C, row.args[1], H, W, row.args[2], 2 * C) == row.route, row.id
        finally:
            for n, v in prev:
                getattr(lib, f"yolosod_debug_set_{n}")(v)
        if row.route.startswith("decomposed"):
            want = 128 if row in br.TILE128_ROWS else 64
            assert [_hip.gemm_bf16_tile(m, n) for m, n in br.swin_gemms(row)] == [want] * 5, row.id
    for row in br.ROWS:
        C = row.shape[1]
        L = br.attn_len(row)
        assert _hip.attention_bf16_form(L, C, br.heads_of(row)) == br.attn_form(L, C, br.heads_of(row)), row.id
    forms = {_hip.attention_bf16_form(*c) for c in br.ATTN_CASES}
    assert None not in forms
    # every compiled key-block count of hd 64: 10 (129..160 keys) is the A2_Attn row with L = 160
    forms |= {_hip.attention_bf16_form(br.attn_len(r), r.shape[1], br.heads_of(r)) for r in br.ROWS}
    assert {n for hd, n in forms if hd == 64} == {4, 6, 8, 10, 12, 16, 20}
    assert len({n for hd, n in forms if hd == 32}) >= 3 and len({n for hd, n in forms if hd == 128}) >= 3
    assert all(_hip.attention_bf16_form(*c) == br.attn_form(*c) for c in br.ATTN_CASES)
    # refusals: hd 128 beyond 192 keys (no instance fits LDS), L > 320, a head dim without a kernel
    assert _hip.attention_bf16_form(*br.ATTN_REFUSED) is None
    assert _hip.attention_bf16_form(192, 256, 2) == (128, 12)
    assert _hip.attention_bf16_form(321, 128, 2) is None and _hip.attention_bf16_form(49, 96, 2) is None
    assert _hip.swin_bf16_route(1, 96, 3, 9, 16, 7, 192) is None      # C % 64
    assert _hip.swin_bf16_route(1, 256, 2, 16, 16, 16, 512) is None   # one 256-token window of hd 128
    assert _hip.swin_bf16_route(0, 64, 2, 9, 16, 7, 128) is None
    # the tile rule at its threshold: 512 tiles of 128x128
    assert _hip.gemm_bf16_tile(4000, 2040) == 128 and _hip.gemm_bf16_tile(4000, 2042) == 128
    assert _hip.gemm_bf16_tile(1000, 1024, 8) == 128 and _hip.gemm_bf16_tile(1000, 1024, 7) == 64
    assert _hip.gemm_bf16_tile(3968, 2040) == 64 and _hip.gemm_bf16_tile(100000, 64) == 64
