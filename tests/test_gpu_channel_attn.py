"""GPU: SE, CBAM and CA (csrc/channel_attention.hip) and the producers of their plane statistics at the shapes, tails and
inputs the fixtures never reach.

Inputs are tests/channel_ref.py's ``structured`` tensors (entirely negative planes, pixels negative in every channel,
offset planes, outliers on both sides of every part boundary), parameters come from recipes.perturb_. Every fp32 output
is held to   |y - ref64| <= K E32 + 2^-23 |ref64|   (ref64 the fp64 oracle, E32 the error of the same oracle in fp32 on
the CPU, K = channel_ref.K for all three ops); tests/test_channel_attn_cpu.py shows that a kernel which started a max
from 0, left the border map non-zero, dropped a part, averaged over the padded length, mis-gated a channel tail, skipped
a short group or lost the column sums past 256 would break it. bf16 storage keeps the bound of tests/test_gpu_bf16.py.
A NaN activation must reach exactly the outputs it reaches in the oracle. Ratios go to YOLOSOD_PARITY_LOG."""
import os

import pytest
import torch

import channel_ref as cr
import recipes
from oplib import tol_close
from yolosod_amd import _hip
from yolosod_amd.nn import modules as M

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _log(msg):
    print(msg)
    log = os.environ.get("YOLOSOD_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?')}: {msg}\n")


def _module(op, arg, C, cuda):
    return cr.build(op, arg, C).to(cuda)


def _run(m, x, cuda):
    with torch.inference_mode():
        return m(x.to(cuda)).cpu()


def _hold(what, y, ref64, e32):
    """Log the ratio to E32 (what K is chosen from) and assert the bound."""
    assert y.dtype == torch.float32 and y.shape == ref64.shape
    r = cr.worst_ratio(y, ref64, e32)
    _log(f"family {what}: worst ratio {cr.e32_ratio(y, ref64, e32):.3f} of E32 {e32:.3g}, {r:.3f} of the bound")
    assert r <= 1.0, f"{what}: |y - ref64| reaches {r:.3f} of {cr.K:g} E32 + 2^-23 |ref64|"


ALL = [(op, c) for op, cases in cr.CASES.items() for c in cases]


@pytest.mark.parametrize("op,case", ALL, ids=[f"{op}-{cr.case_id(c)}" for op, c in ALL])
def test_structured_inputs_vs_oracle(op, case, cuda):
    shape, arg, _ = case
    x, ref64, e32 = cr.case_data(op, shape, arg)
    _hold(f"{op} {cr.case_id(case)}", _run(_module(op, arg, shape[1], cuda), x, cuda), ref64, e32)


STARRED = [(op, c) for op, c in ALL if c[2]]


@pytest.mark.parametrize("op,case", STARRED, ids=[f"{op}-{cr.case_id(c)}" for op, c in STARRED])
def test_structured_inputs_bf16_storage(op, case, cuda):
    """bf16 storage against the fp64 oracle on the bf16-rounded parameters and input: tests/test_gpu_bf16.py's bound."""
    shape, arg, _ = case
    x = cr.case_data(op, shape, arg)[0]
    m = _module(op, arg, shape[1], cuda).to(BF)
    with torch.inference_mode():
        y = m(x.to(cuda).to(BF))
    assert y.dtype == BF
    ref = cr.oracle_bf16(op, arg, x)
    d = (y.double().cpu() - ref).abs()
    lim = 2.0 ** -7 * ref.abs() + 1e-6 * float(ref.abs().max())
    _log(f"family {op} bf16 {cr.case_id(case)}: max|d| {float(d.max()):.3g} ratio {float((d / lim).max()):.3f}")
    assert bool((d <= lim).all()), f"max|d| {float(d.max()):.3g}, worst ratio {float((d / lim).max()):.2f}"


@pytest.mark.parametrize("case", cr.SE_GATE_CASES, ids=cr.case_id)
def test_se_gate_vs_oracle(case, cuda):
    shape, arg, _ = case
    x = cr.case_data("SE_Block", shape, arg)[0]
    (g64, e32), = cr.oracle_gates("SE_Block", arg, x)
    m = _module("SE_Block", arg, shape[1], cuda)
    with torch.inference_mode():
        g = m.gate(x.to(cuda)).cpu()
    _hold(f"SE.gate {cr.case_id(case)}", g, g64, e32)


@pytest.mark.parametrize("case", cr.CBAM_GATE_CASES, ids=cr.case_id)
def test_cbam_gates_vs_oracle(case, cuda):
    shape, arg, _ = case
    x = cr.case_data("CBAM_Block", shape, arg)[0]
    (ca64, eca), (sa64, esa) = cr.oracle_gates("CBAM_Block", arg, x)
    m = _module("CBAM_Block", arg, shape[1], cuda)
    with torch.inference_mode():
        ca, sa = m.gates(x.to(cuda))
    _hold(f"CBAM.gates ca {cr.case_id(case)}", ca.cpu(), ca64, eca)
    _hold(f"CBAM.gates sa {cr.case_id(case)}", sa.cpu(), sa64, esa)


# ---- producers at parts > 1 -----------------------------------------------------------------------------------------

def _check_stats(what, out, plain, stats, cuda):
    """The four checks of a statistics launch, then SE (and, with maxes, CBAM) fed with the partials."""
    B, C, H, W = out.shape
    assert torch.equal(out, plain), what
    st = out._ys_plane_stats
    assert st.parts == _hip.plane_parts(H * W)[0] == cr.part_plan(H * W)[0]
    o64 = out.double()
    ref, lim = o64.sum((2, 3)), H * W * 2.0 ** -24 * o64.abs().sum((2, 3))
    err = (st.psum.view(B, C, st.parts).double().sum(2) - ref).abs()
    _log(f"family {what}: sum err / bound {float((err / lim).max()):.3g}")
    assert bool((err <= lim).all()), (what, float((err / lim).max()))
    top = out.amax((2, 3))
    if stats == "summax":
        assert bool((top < 0).any()), "no entirely negative plane in this case"
        assert torch.equal(st.pmax.view(B, C, st.parts).amax(2), top), what
    else:
        assert st.pmax is None
    se = M.SE_Block(4)
    se._maybe_build(C, None)
    mods = [se] + ([M.CBAM_Block(C, None, 4)] if stats == "summax" else [])
    for m in mods:
        recipes.perturb_(m, 3)
        m.to(cuda).eval()
        with torch.inference_mode():
            a, b = m(plain), m(out)
        ok, e, _ = tol_close(b.cpu(), a.cpu(), 1e-6, 1e-5)
        assert ok, (what, type(m).__name__, e)


@pytest.mark.parametrize("stats", ["sum", "summax"])
@pytest.mark.parametrize("shape", [(1, 8, 128, 128), (1, 8, 131, 127), (1, 8, 172, 143)],
                         ids=lambda s: "x".join(map(str, s)))
def test_bias_act_stats_multi_part(shape, stats, cuda):
    """bias_act(stats=...) on planes of 2 and 3 parts; every third plane has y + bias in [-1.2, -0.2], entirely negative
    after SiLU. The epilogue kernels move 4 elements per access: a plane with H W % 4 != 0 (131 x 127) is refused by
    the plain and the statistics entry points alike (Conv runs such maps through torch), before anything launches."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(H + W)
    y = torch.randn(shape, generator=g)
    bias = torch.randn(C, generator=g)
    y[:, 2::3] = -(torch.rand(B, len(range(2, C, 3)), H, W, generator=g) + 0.2) - bias[2::3].view(1, -1, 1, 1)
    y, bias = y.to(cuda), bias.to(cuda)
    if (H * W) % 4:
        for kw in ({}, {"stats": stats}):
            before = y.clone()
            with pytest.raises(RuntimeError, match="must be multiples of 4"):
                _hip.bias_act(y, bias, 1, **kw)
            assert torch.equal(y, before)
        return
    plain = _hip.bias_act(y.clone(), bias, 1)
    out = _hip.bias_act(y.clone(), bias, 1, stats=stats)
    assert out._ys_plane_stats.parts > 1
    _check_stats(f"bias_act_stats {shape} {stats}", out, plain, stats, cuda)


def _conv_case(cin, cout, seed):
    """x, w, bias of a 1x1 conv at 128 x 128 (2 parts); every third output plane is entirely negative after SiLU."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, cin, 128, 128, generator=g)
    w = torch.randn(cout, cin, generator=g) / cin ** 0.5
    b = torch.randn(cout, generator=g)
    w[2::3] *= 0.02   # pre-activations of these rows: -0.7 +- 0.1
    b[2::3] = -0.7
    return x, w, b


@pytest.mark.parametrize("stats", ["sum", "summax"])
def test_conv1x1_thin_stats_multi_part(stats, cuda):
    x, w, b = (t.to(cuda) for t in _conv_case(64, 64, 5))
    plain = _hip.conv1x1_thin(x, w, b)
    out = _hip.conv1x1_thin(x, w, b, stats=stats)
    _check_stats(f"conv1x1_thin_stats 64->64 {stats}", out, plain, stats, cuda)


@pytest.mark.parametrize("stats", ["sum", "summax"])
def test_conv1x1x2_stats_multi_part(stats, cuda):
    x, w, b = (t.to(cuda) for t in _conv_case(192, 128, 6))
    prep = _hip.conv1x1x2_prepare(w)
    _hip.split_range_flag(reset=True)
    plain = _hip.conv1x1x2_silu(x, b, lambda: prep, 128)
    out = _hip.conv1x1x2_silu(x, b, lambda: prep, 128, stats=stats)
    assert not _hip.split_range_flag(reset=True)
    _check_stats(f"conv1x1x2_stats 192->128 {stats}", out, plain, stats, cuda)


# ---- limits -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("op,arg,shape,msg", [
    ("SE_Block", 2, (1, 130, 4, 4), "se: hidden=65 unsupported"),
    ("CBAM_Block", 2, (1, 130, 4, 4), "cbam: hidden=65 unsupported"),
    ("CA_Block", 32, (1, 8, 2, 1025), r"ca: bad shape \(W <= 1024 supported\)"),
    ("CA_Block", 32, (1, 2080, 4, 4), "ca: mip=65 unsupported"),
], ids=["se_hid65", "cbam_hid65", "ca_w1025", "ca_mip65"])
def test_limits_raise_before_any_launch(op, arg, shape, msg, cuda):
    m = _module(op, arg, shape[1], cuda)
    x = torch.randn(shape, device=cuda)
    with pytest.raises(RuntimeError, match=msg):
        with torch.inference_mode():
            m(x)
    torch.cuda.synchronize()


# ---- NaN propagation ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", list(cr.CASES))
@pytest.mark.parametrize("shape", cr.NAN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_nan_reaches_what_it_reaches_in_the_oracle(op, shape, cuda):
    """One NaN at x[1, 3, 2, 4]: the NaN mask of y is the oracle's, image 0 keeps its bits."""
    arg = cr.NAN_ARG[op]
    x = cr.structured(shape, 11)
    xn = cr.with_nan(x)
    mask = torch.isnan(cr.oracle(op, arg, xn)[0])
    assert bool(mask[1].any()) and not bool(mask[0].any())
    m = _module(op, arg, shape[1], cuda)
    y, yn = _run(m, x, cuda), _run(m, xn, cuda)
    assert not bool(torch.isnan(y).any())
    got = torch.isnan(yn)
    assert torch.equal(got, mask), f"{op} {shape}: {int(got.sum())} NaN outputs, the oracle has {int(mask.sum())}"
    assert torch.equal(yn[0], y[0])


@pytest.mark.parametrize("op", ["SE_Block", "CBAM_Block"])
@pytest.mark.parametrize("shape", cr.NAN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_nan_reaches_the_gates(op, shape, cuda):
    arg = cr.NAN_ARG[op]
    x = cr.structured(shape, 11)
    xn = cr.with_nan(x)
    masks = [torch.isnan(g) for g, _ in cr.oracle_gates(op, arg, xn)]
    m = _module(op, arg, shape[1], cuda)

    def gates(t):
        with torch.inference_mode():
            g = m.gate(t.to(cuda)) if op == "SE_Block" else m.gates(t.to(cuda))
        return [v.cpu() for v in (g if isinstance(g, tuple) else (g,))]

    for g, gn, mask in zip(gates(x), gates(xn), masks):
        assert bool(mask[1].all()) and not bool(mask[0].any())
        assert torch.equal(torch.isnan(gn), mask)
        assert torch.equal(gn[0], g[0])


def _check_nan_pmax(out):
    """The merged partial max of every plane is NaN exactly where the plane holds a NaN, and the plane max elsewhere."""
    B, C = out.shape[:2]
    st = out._ys_plane_stats
    merged = st.pmax.view(B, C, st.parts).amax(2)      # amax hands a NaN on, like the gate's merge
    top = out.amax((2, 3))
    assert bool(torch.isnan(top[1]).any()) and not bool(torch.isnan(top[0]).any())
    assert torch.equal(torch.isnan(merged), torch.isnan(top))
    assert torch.equal(torch.nan_to_num(merged, nan=0.0), torch.nan_to_num(top, nan=0.0))


def test_nan_reaches_the_producers_pmax(cuda):
    g = torch.Generator().manual_seed(2)
    y = torch.randn(2, 8, 128, 128, generator=g)
    y[cr.NAN_AT] = float("nan")
    out = _hip.bias_act(y.to(cuda), torch.randn(8, generator=g).to(cuda), 1, stats="summax")
    assert int(torch.isnan(out.amax((2, 3))).sum()) == 1
    _check_nan_pmax(out)
    # a NaN input pixel of a 1x1 conv is a NaN in every output plane of that image
    x = torch.randn(2, 64, 16, 24, generator=g)
    x[cr.NAN_AT] = float("nan")
    w, b = torch.randn(64, 64, generator=g) / 8, torch.randn(64, generator=g)
    _check_nan_pmax(_hip.conv1x1_thin(x.to(cuda), w.to(cuda), b.to(cuda), stats="summax"))
    x = torch.randn(2, 192, 12, 12, generator=g)
    x[cr.NAN_AT] = float("nan")
    w, b = torch.randn(128, 192, generator=g) / 192 ** 0.5, torch.randn(128, generator=g)
    prep = _hip.conv1x1x2_prepare(w.to(cuda))
    _hip.split_range_flag(reset=True)
    out = _hip.conv1x1x2_silu(x.to(cuda), b.to(cuda), lambda: prep, 128, stats="summax")
    assert _hip.split_range_flag(reset=True)           # the split-range guard reports the NaN too
    _check_nan_pmax(out)
