"""GPU: SwinBlock on each of its four fp32 routes, A2_Attn in its four forms, MambaBlock and the layernorm / attention
pieces against the fp64 oracle, held to  |y - ref64| <= K E32 + 2^-23 |ref64|  (tests/attn_ref.py)
on random, structured, all-zero and peaked-softmax inputs and with a NaN or +Inf in the input; the route report
(yolosod_debug_swin_route / yolosod_debug_swin_last_route) shows that every row ran where the table says."""
import contextlib
import functools

import pytest
import torch

import attn_ref as ar
from yolosod_amd import _hip

pytestmark = pytest.mark.gpu

NAN_ROWS = [r for r in ar.ROWS if r.shape != (1, 512, 9, 9)]  # NaN share 0.605 there (tests/test_attn_family_cpu.py)
# one row per route for the batch test
BATCH_ROWS = ([ar.SWIN_ROWS[i] for i in (0, 1, 2, 6, 11, 12, 14, 16)] + ar.A2_ROWS[:4] + ar.A2_ROWS[8:9]
              + ar.MAMBA_ROWS[:1])


@contextlib.contextmanager
def switched(row):
    """The row's switches set, and put back whatever happens."""
    lib = _hip.load_library()
    undo = []
    try:
        for name, v in row.switches:
            prev = getattr(lib, f"yolosod_debug_set_{name}")(v)
            undo.append((name, 1 if prev is None else prev))  # set_swin_fused returns nothing; its default is 1
        yield
    finally:
        for name, v in undo:
            getattr(lib, f"yolosod_debug_set_{name}")(v)


@functools.lru_cache(maxsize=None)
def _module(op, args, sharp, dev):
    return ar.build(op, args, sharp).to(dev)


def run(row, x, cuda, sharp=False):
    """y of the row's module on its route; for SwinBlock the route is asserted on the way."""
    m = _module(row.op, row.args, sharp, cuda)
    with switched(row), torch.inference_mode():
        if row.route is not None:
            B, C, H, W = x.shape
            assert _hip.swin_route(B, C, row.args[1], H, W, row.args[2], 2 * C) == row.route
        y = m(x.to(cuda)).cpu()
        if row.route is not None:
            assert _hip.swin_last_route() == row.route, (row.id, _hip.swin_last_route())
    return y


def _cases(rows):
    return [pytest.param(r, k, id=f"{r.id}-{k}") for r in rows for k in ar.inputs_of(r)]


@pytest.mark.parametrize("row,kind", _cases(ar.ROWS))
def test_parity_on_every_route(row, kind, cuda):
    x, ref = ar.case_data(row.op, row.args, row.shape, kind)
    y = run(row, x, cuda, kind == "sharp")
    print(f"family {row.id} {kind}: kernel ratio to E32 {ar.e32_ratio(y, ref.ref64, ref.e32):.3f} (E32 {ref.e32:.3g})")
    r = ar.worst_ratio(y, ref.ref64, ref.e32)
    assert r <= 1.0, (row.id, kind, r)


@pytest.mark.parametrize("group", ar.CROSS, ids=lambda g: f"{g[0].op}-{'x'.join(map(str, g[0].shape))}")
def test_routes_agree_with_each_other(group, cuda):
    """The routes that run the same (module, input) differ by at most twice the bound."""
    for kind in ar.inputs_of(group[0]):
        x, ref = ar.case_data(group[0].op, group[0].args, group[0].shape, kind)
        ys = [run(r, x, cuda, kind == "sharp") for r in group]
        lim = 2.0 * ar.bound(ref.ref64, ref.e32)
        for i in range(len(ys)):
            for j in range(i + 1, len(ys)):
                d = (ys[i].double() - ys[j].double()).abs()
                print(f"family cross {group[i].id} / {group[j].id} {kind}: {float((d / lim).max()):.3f} of 2 x bound")
                assert bool((d <= lim).all()), (group[i].id, group[j].id, kind, float((d / lim).max()))


@pytest.mark.parametrize("special", ["nan", "inf"])
@pytest.mark.parametrize("row", NAN_ROWS, ids=lambda r: r.id)
def test_nan_and_inf_reach_the_output_as_in_the_oracle(row, special, cuda):
    """NaN or +Inf at x[0, 3, 2, 4]: the output is NaN (not finite) exactly where the oracle's is and within the bound
    everywhere else; the fp16-split routes leave the split-range flag set."""
    x, ref = ar.case_data(row.op, row.args, row.shape, "structured", special)
    _hip.split_range_flag(reset=True, device=cuda)
    y = run(row, x, cuda)
    flag = _hip.split_range_flag(reset=True, device=cuda)
    yn, rn = ~torch.isfinite(y), torch.isnan(y)
    want = torch.isnan(ref.ref64) if special == "nan" else ref.nonfinite32
    got = rn if special == "nan" else yn
    print(f"family {row.id} {special}: mask {int(got.sum())} of oracle's {int(want.sum())}, "
          f"missing {int((want & ~got).sum())}, extra {int((got & ~want).sum())}, flag {flag}")
    assert torch.equal(got, want), (row.id, special, int((want & ~got).sum()), int((got & ~want).sum()))
    r = ar.worst_ratio(y, ref.ref64, ref.e32, nonfinite=None if special == "nan" else ref.nonfinite32)
    assert r <= 1.0, (row.id, special, r)
    if row.route == "split_fused" or dict(row.switches).get("a2_x2") == 1:
        assert flag, row.id


@pytest.mark.parametrize("row", ar.LOCALITY, ids=lambda r: r.id)
def test_swin_windows_do_not_see_each_other(row, cuda):
    """Pixels changed strictly inside one window, two or more pixels from its border (the depthwise 3x3 stays inside),
    change no output bit of any other window."""
    x, _ = ar.case_data(row.op, row.args, row.shape, "structured")
    img = row.shape[0] - 1
    x2 = x.clone()
    g = torch.Generator().manual_seed(5)
    x2[img, :, 9:12, 2:5] += torch.randn(row.shape[1], 3, 3, generator=g)  # window (wy 1, wx 0): rows 7..13, cols 0..6
    y, y2 = run(row, x, cuda), run(row, x2, cuda)
    others = torch.ones(row.shape, dtype=torch.bool)
    others[img, :, 7:14, 0:7] = False
    assert torch.equal(y[others], y2[others]), int((y != y2)[others].sum())
    assert not torch.equal(y[~others], y2[~others])


@pytest.mark.parametrize("row", BATCH_ROWS, ids=lambda r: r.id)
def test_batch_invariance(row, cuda):
    """m(x) is bitwise cat(m(x[i:i+1])) at B = 3 on every route."""
    shape = (3,) + row.shape[1:]
    x = torch.randn(shape, generator=torch.Generator().manual_seed(17))
    a = run(row, x, cuda)
    b = torch.cat([run(row, x[i:i + 1], cuda) for i in range(3)])
    assert torch.equal(a, b), float((a - b).abs().max())


# ---- the pieces -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["constant", "offset", "nan"])
@pytest.mark.parametrize("C", [32, 96, 1000])
def test_layernorm_rows(C, kind, cuda):
    """_hip.layernorm on rows that are constant (variance 0: the eps path), 1e3 + randn (cancellation in x - mean) and
    randn with one NaN (that row NaN, the others bitwise as without it)."""
    rows = 67
    g = torch.Generator().manual_seed(C)
    x = torch.randn(rows, C, generator=g)
    if kind == "constant":
        x = torch.randn(rows, 1, generator=g).expand(rows, C).contiguous() * 3
    elif kind == "offset":
        x = x + 1e3
    w, b = 1.0 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    ln = torch.nn.functional.layer_norm
    ref64 = ln(x.double(), (C,), w.double(), b.double(), 1e-5)
    e32 = float((ln(x, (C,), w, b, 1e-5).double() - ref64).abs().max())
    y = _hip.layernorm(x.to(cuda), w.to(cuda), b.to(cuda), 1e-5).cpu()
    if kind == "nan":
        xn = x.clone()
        xn[5, C // 3] = float("nan")
        yn = _hip.layernorm(xn.to(cuda), w.to(cuda), b.to(cuda), 1e-5).cpu()
        assert bool(torch.isnan(yn[5]).all())
        keep = torch.arange(rows) != 5
        assert torch.equal(yn[keep], y[keep])
    print(f"family layernorm C={C} {kind}: kernel ratio to E32 {ar.e32_ratio(y, ref64, e32) if e32 else 0.0:.3f} "
          f"(E32 {e32:.3g})")
    assert ar.worst_ratio(y, ref64, e32) <= 1.0


@pytest.mark.parametrize("L,C,heads", [(30, 256, 4), (35, 64, 4), (49, 96, 3), (81, 512, 4)])
def test_attention_peaked_and_nan(L, C, heads, cuda):
    """_hip.attention with q and k scaled by 4 (peaked rows) against the fp64 restatement; a NaN in one key row of one
    sequence, inside one head, makes that (sequence, head) NaN and leaves every other output bit as without it."""
    nseq, hd = 3, C // heads
    qkv = torch.randn(nseq * L, 3 * C, generator=torch.Generator().manual_seed(L * 31 + C))
    qkv[:, :2 * C] *= 4.0
    ref64 = ar.attention_ref(qkv.double(), nseq, L, C, heads)
    e32 = float((ar.attention_ref(qkv, nseq, L, C, heads).double() - ref64).abs().max())
    y = _hip.attention(qkv.to(cuda), nseq, L, C, heads).cpu()
    print(f"family attention L={L} C={C} heads={heads}: kernel ratio to E32 {ar.e32_ratio(y, ref64, e32):.3f} "
          f"(E32 {e32:.3g})")
    assert ar.worst_ratio(y, ref64, e32) <= 1.0
    qn = qkv.clone()
    qn[1 * L + 7, C + 1 * hd + 3] = float("nan")  # sequence 1, key 7, head 1
    yn = _hip.attention(qn.to(cuda), nseq, L, C, heads).cpu()
    want = torch.zeros(nseq * L, C, dtype=torch.bool)
    want[L:2 * L, hd:2 * hd] = True
    assert torch.equal(torch.isnan(yn), want), (int(torch.isnan(yn).sum()), int(want.sum()))
    assert torch.equal(yn[~want], y[~want])
