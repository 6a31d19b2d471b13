"""GPU: the fp16-split conv kernels held to the split's a-priori error budget (tests/split_budget.py, DESIGN.md
section 4) across magnitudes: activations at scale 1, 2^-3, 2^-6 and 1e-3, flat and with per-channel scales of
2^-10 .. 2^2 on activations and weights, and a bias that follows the signal. The bound is

    |y - ref64| <= 8 E32 + 1.1 F        (elementwise, no additive slack)

with E32 the error of torch's fp32 conv on the CPU and F = sum_k 2^-25 |w_nk| + 2^-31 |x_k| the representation floor of
the two-term split. tests/test_split_budget_cpu.py shows that a kernel which loses a low-term product, flushes the
subnormal low terms, or loses one tap's or one 32-channel chunk's low terms breaks this bound at scales >= 2^-6.

Every tile / group form the shape admits is forced and must be bit-identical to the first at every scale; the
split-range flag stays clear throughout. Worst ratios go to YOLOSOD_PARITY_LOG (MIOpen's own fp32 error beside them,
for information: it is not in the bound)."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import split_budget as sb
from yolosod_amd import _hip

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S3, S6 = 2.0 ** -3, 2.0 ** -6


def _log(msg):
    print(msg)
    log = os.environ.get("YOLOSOD_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?')}: {msg}\n")


class _hook:
    """``with _hook(setter, value)``: a debug switch of the library that returns its previous value, restored on
    exit."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = getattr(_hip.load_library(), self.name)(self.value)

    def __exit__(self, *exc):
        getattr(_hip.load_library(), self.name)(self.old)
        return False


def _kind(case):
    k, stride = case[5], case[6]
    return "conv1x1x2" if k == 1 else ("conv3x3s2" if stride == 2 else "conv3x3")


def _forms(case):
    """(setter, [forms]) of a case: every form its shape admits, as the *_forms.py / *_c32.py tests enumerate them;
    [0] where the launch has one form only (the automatic setting)."""
    B, cin, cout, H, W, k, stride = case
    kind = _kind(case)
    if kind == "conv3x3":
        if W % 4:  # the one-tile-per-workgroup kernel
            return "yolosod_debug_set_conv3x3_form", [0]
        grps = (2, 3, 4) if (cin, cout) == (32, 32) else (2,) if cout == 32 else (1, 2)
        return "yolosod_debug_set_conv3x3_form", [g + 4 * grp for g in (1, 2, 3) for grp in grps]
    if kind == "conv3x3s2":
        if (cin, cout) == (32, 64):  # the register-weight kernel
            return "yolosod_debug_set_conv3x3s2_form", [0]
        return "yolosod_debug_set_conv3x3s2_form", [g + 4 * grp for g in (1, 2, 3)
                                                    for grp in ((2,) if cout == 64 else (1, 2))]
    return "yolosod_debug_set_conv1x1x2_form", [1 + 4, 2 + 4, 1 + 8, 2 + 8] if cout % 256 == 0 else [1 + 4, 1 + 8]


def _resolved(case, form):
    """The form the library reports for the case under the current setting (0: a launch with one form only)."""
    B, cin, cout, H, W, k, stride = case
    lib = _hip.load_library()
    kind = _kind(case)
    if kind == "conv3x3":
        return lib.yolosod_debug_conv3x3_form_ex(B, cin, cout, H, W)
    if kind == "conv3x3s2":
        return form if form == 0 else lib.yolosod_debug_conv3x3s2_form(B, cout, H, W)
    return lib.yolosod_debug_conv1x1x2_form(B, cout, H, W)


def _prepare(case, wd):
    return {"conv3x3": _hip.conv3x3_prepare, "conv3x3s2": _hip.conv3x3s2_prepare,
            "conv1x1x2": _hip.conv1x1x2_prepare}[_kind(case)](wd)


def _run(case, xd, bd, prep, gc=None, gp=None):
    kind, cout = _kind(case), case[2]
    if kind == "conv3x3":
        return _hip.conv3x3_silu(xd, bd, lambda: prep, cout)
    if kind == "conv3x3s2":
        return _hip.conv3x3s2_silu(xd, bd, lambda: prep, cout, gc, gp)
    return _hip.conv1x1x2_silu(xd, bd, lambda: prep, cout)


def _miopen_err(x_eff, w, b, k, stride, ref64):
    y = F.silu(F.conv2d(x_eff.to(DEV), w.to(DEV), b.to(DEV), stride=stride, padding=k // 2))
    return float((y.cpu().double() - ref64).abs().max())


def _check_budget(y, ref64, lim, what):
    yc = y.cpu()
    assert yc.shape == ref64.shape, (what, tuple(yc.shape))
    assert bool(torch.isfinite(yc).all()), what
    r = sb.worst_ratio(yc, ref64, lim)
    assert r <= 1.0, f"{what}: |y - ref64| reaches {r:.3f} of 8 E32 + 1.1 F"
    return r


# ---- a. the conv kernels against the budget, every form ----------------------------------------------------------

@pytest.mark.parametrize("case", sb.CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_kernels_keep_the_budget_in_every_form(case, cuda):
    k, stride = case[5], case[6]
    setter, forms = _forms(case)
    worst = 0.0
    for s, wide in sb.variants():
        x, w, b = sb.make_case(*case, s, wide)
        ref64, lim = sb.budget(x, w, b, k, stride)
        xd, bd = x.to(cuda), b.to(cuda)
        _hip.split_range_flag(reset=True)
        prep = _prepare(case, w.to(cuda))
        y0 = None
        for form in forms:
            with _hook(setter, form):
                assert _resolved(case, form) == form, (case, form)
                y = _run(case, xd, bd, prep)
            what = f"{_kind(case)} {case} s={s:.3g} wide={wide} form {form}"
            r = _check_budget(y, ref64, lim, what)
            if y0 is None:
                y0 = y
                e_m = _miopen_err(x, w, b, k, stride, ref64)
                e32 = float((F.silu(F.conv2d(x, w, b, stride=stride, padding=k // 2)).double() - ref64).abs().max())
                e = float((y.cpu().double() - ref64).abs().max())
                _log(f"{what}: ratio {r:.3f}, max|err| {e:.3g} (E32 {e32:.3g}, MIOpen fp32 {e_m:.3g})")
                worst = max(worst, r)
            assert torch.equal(y, y0), f"{what} differs from form {forms[0]}"
        assert not _hip.split_range_flag(reset=True), (case, s, wide)
    _log(f"family {_kind(case)} {case}: worst ratio {worst:.3f} over {len(forms)} form(s)")


# ---- b. the stride-2 kernel's gates --------------------------------------------------------------------------------

@pytest.mark.parametrize("gates", ["c", "p", "cp"])
@pytest.mark.parametrize("case", [(2, 32, 64, 17, 39, 3, 2), (1, 96, 128, 8, 8, 3, 2)],
                         ids=lambda c: "x".join(map(str, c)))
def test_stride2_gates_keep_the_budget(case, gates, cuda):
    """The gated operand (x * gate_c) * gate_p, gates in (0, 1), is where a small value is most likely: the
    register-weight kernel (Cin 32 -> Cout 64) and every form of the tiled kernel (Cin 96 -> Cout 128), at s = 2^-6."""
    B, cin, cout, H, W, k, stride = case
    x, w, b = sb.make_case(*case, S6, False)
    g = torch.Generator().manual_seed(sum(case) + len(gates) + 100 * ("c" in gates))
    gc = torch.sigmoid(torch.randn(B, cin, generator=g)) if "c" in gates else None
    gp = torch.sigmoid(torch.randn(B, H, W, generator=g)) if "p" in gates else None
    ref64, lim = sb.budget(x, w, b, k, stride, gate_c=gc, gate_p=gp)
    d = lambda t: None if t is None else t.to(cuda)  # noqa: E731
    xd, bd, gcd, gpd = d(x), d(b), d(gc), d(gp)
    _hip.split_range_flag(reset=True)
    prep = _hip.conv3x3s2_prepare(w.to(cuda))
    setter, forms = _forms(case)
    y0, worst = None, 0.0
    for form in forms:
        with _hook(setter, form):
            assert _resolved(case, form) == form, (case, form)
            y = _run(case, xd, bd, prep, gcd, gpd)
        worst = max(worst, _check_budget(y, ref64, lim, f"conv3x3s2 {case} gates {gates} form {form}"))
        y0 = y if y0 is None else y0
        assert torch.equal(y, y0), (case, gates, form)
    assert not _hip.split_range_flag(reset=True)
    _log(f"family conv3x3s2_gates {case} gates {gates} s=2^-6: worst ratio {worst:.3f} over {len(forms)} form(s)")


# ---- c. the statistics forms of the 1x1 kernel -----------------------------------------------------------------------

@pytest.mark.parametrize("stats", ["sum", "summax"])
def test_statistics_forms_at_small_scale(stats, cuda):
    """The stored output is the plain launch's bit for bit; the max is the max of the stored values; the sum keeps the
    bound of tests/test_gpu_conv1x1x2_stats.py (HW fp32 additions: HW 2^-24 sum|out|)."""
    case = (1, 384, 256, 12, 12, 1, 1)
    B, cin, cout, H, W, k, stride = case
    x, w, b = sb.make_case(*case, S6, False)
    xd, bd = x.to(cuda), b.to(cuda)
    prep = _hip.conv1x1x2_prepare(w.to(cuda))
    _hip.split_range_flag(reset=True)
    for form in (1 + 4, 2 + 4):  # the routed forms of the statistics launch
        with _hook("yolosod_debug_set_conv1x1x2_form", form):
            y0 = _hip.conv1x1x2_silu(xd, bd, lambda: prep, cout)
            y = _hip.conv1x1x2_silu(xd, bd, lambda: prep, cout, stats=stats)
        assert torch.equal(y, y0), form
        st = y._ys_plane_stats
        assert st.parts == _hip.plane_parts(H * W)[0]
        ps = st.psum.view(B, cout, st.parts)
        y64 = y.double()
        ref, bound = y64.sum((2, 3)), H * W * 2.0 ** -24 * y64.abs().sum((2, 3))
        err = (ps.double().sum(2) - ref).abs()
        assert bool((err <= bound).all()), (form, float((err / bound).max()))
        if stats == "summax":
            assert torch.equal(st.pmax.view(B, cout, st.parts).amax(2), y.amax((2, 3))), form
        else:
            assert st.pmax is None
        _log(f"family conv1x1x2_stats {case} {stats} form {form} s=2^-6: sum err / bound "
             f"{float((err / bound).max()):.3f}")
    assert not _hip.split_range_flag(reset=True)


# ---- d. the fused Bottleneck -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("s,wide", [(S3, False), (S6, False), (S6, True)])
def test_fused_bottleneck_equals_two_launches(s, wide, cuda):
    """One launch against two conv3x3_silu launches, bit for bit (the budget of that form: test a, Cin 32 ->
    Cout 32)."""
    x, w1, b1 = sb.make_case(2, 32, 32, 12, 20, 3, 1, s, wide)
    _, w2, b2 = sb.make_case(1, 32, 32, 12, 20, 3, 1, s, wide)  # another seed: the second conv's weights
    xd, b1d, b2d = x.to(cuda), b1.to(cuda), b2.to(cuda)
    p1, p2 = _hip.conv3x3_prepare(w1.to(cuda)), _hip.conv3x3_prepare(w2.to(cuda))
    _hip.split_range_flag(reset=True)
    t = _hip.conv3x3_silu(xd, b1d, lambda: p1, 32)
    for res in (False, True):
        pair = _hip.conv3x3_silu(t, b2d, lambda: p2, 32, res=xd if res else None)
        with _hook("yolosod_debug_set_bottleneck3x3_fuse", 1):
            assert _hip.bottleneck3x3_fused(2, 12, 20)
            y = _hip.bottleneck3x3_silu(xd, b1d, lambda: p1, b2d, lambda: p2, res=xd if res else None)
        assert torch.equal(y, pair), (s, wide, res, float((y - pair).abs().max()))
    assert not _hip.split_range_flag(reset=True)


# ---- e. the Detect head, signal-relative -----------------------------------------------------------------------------

NC, HEAD_STRIDE = 10, 8.0
HEAD_VARIANTS = [(1.0, False), (S3, False), (S6, False), (S6, True)]


@functools.lru_cache(maxsize=None)
def _head_case(s, wide):
    """One level of [2, 64, 8, 8] tower features at scale s; class weights randn * 0.2 (wide: per-channel scales of
    2^-10 .. 2^2 on weights and features); the class bias follows the signal, so p ~ 0.5 and the logit is resolvable."""
    g = torch.Generator().manual_seed(64 + 8 + 8 + NC)
    fb = torch.randn(2, 64, 8, 8, generator=g) * s
    fc = torch.randn(2, 64, 8, 8, generator=g) * s
    wb = torch.randn(64, 64, generator=g) * 0.25
    bb = torch.randn(64, generator=g)
    wc = torch.randn(NC, 64, generator=g) * 0.2
    if wide:
        wc = wc * 2.0 ** (torch.rand(NC, 1, generator=g) * 12 - 10)
        fc = fc * 2.0 ** (torch.rand(1, 64, 1, 1, generator=g) * 12 - 10)
    bc = 0.1 * fc.abs().mean() * torch.randn(NC, generator=g)
    return fb.contiguous(), fc.contiguous(), wb, bb, wc.contiguous(), bc


def _logit64(p):
    p = p.double()
    return torch.log(p) - torch.log1p(-p)


@pytest.mark.parametrize("s,wide", HEAD_VARIANTS)
def test_detect_head_class_rows_in_logit_space(s, wide, cuda):
    """|logit(y) - z64| <= 8 E32z + Fz on the class rows: z64 the fp64 logits, E32z the error of the fp32 CPU
    restatement (fp32 matmul, torch.sigmoid in fp32, the logit taken in float64), Fz the split's floor for the 1x1 head
    weights (64 W as in the conv kernels, csrc/detect_head_math.h). The box rows are skipped: DFL's softmax makes them
    insensitive to the features at these scales."""
    fb, fc, wb, bb, wc, bc = _head_case(s, wide)
    z64 = torch.einsum("ok,bkhw->bohw", wc.double(), fc.double()) + bc.double().view(1, -1, 1, 1)
    z32 = torch.einsum("ok,bkhw->bohw", wc, fc) + bc.view(1, -1, 1, 1)
    e32z = float((_logit64(torch.sigmoid(z32)) - z64).abs().max())
    fz = (torch.einsum("ok,bkhw->bohw", wc.double().abs(), torch.full_like(fc, sb.X_FLOOR, dtype=torch.float64))
          + torch.einsum("ok,bkhw->bohw", torch.full_like(wc, sb.W_FLOOR, dtype=torch.float64), fc.double().abs()))
    lim = 8.0 * e32z + fz
    d = lambda t: t.to(cuda)  # noqa: E731
    _hip.split_range_flag(reset=True)
    with _hook("yolosod_debug_set_head_x2", 1):
        y = _hip.detect_head([d(fb)], [d(fc)], [d(wb)], [d(bb)], [d(wc)], [d(bc)], [HEAD_STRIDE], NC)
    assert not _hip.split_range_flag(reset=True)
    p = y[:, 4:].cpu().view(2, NC, 8, 8)
    assert bool(((p > 0) & (p < 1)).all())
    err = (_logit64(p) - z64).abs()
    r = float((err / lim).max())
    _log(f"family detect_head s={s:.3g} wide={wide}: logit ratio {r:.3f}, max|dz| {float(err.max()):.3g} "
         f"(E32z {e32z:.3g}, max|z - b| {float((z64 - bc.double().view(1, -1, 1, 1)).abs().max()):.3g})")
    assert r <= 1.0, f"s={s} wide={wide}: |logit(y) - z64| reaches {r:.3f} of 8 E32z + Fz"


@pytest.mark.parametrize("s,wide", HEAD_VARIANTS)
def test_conv3x3_head_class_mode_equals_conv_then_head(s, wide, cuda):
    """conv3x3_head mode 2 on the same level (the fused route forced) against conv3x3_silu followed by
    detect_head_into, bit for bit on the class rows, the way tests/test_gpu_conv3x3_head.py builds its reference."""
    x, w, b = sb.make_case(2, 64, 64, 8, 8, 3, 1, s, wide)
    _, _, _, _, wc, _ = _head_case(s, wide)
    g = torch.Generator().manual_seed(5)
    wb, bb = torch.randn(64, 64, generator=g) * 0.25, torch.randn(64, generator=g)
    xd, bd, wcd = x.to(cuda), b.to(cuda), wc.to(cuda)
    prep = _hip.conv3x3_prepare(w.to(cuda))
    hprep = _hip.detect_head_prepare(wcd, NC)
    _hip.split_range_flag(reset=True)
    f = _hip.conv3x3_silu(xd, bd, lambda: prep, 64)
    bcd = (0.1 * f.abs().mean() * torch.randn(NC, generator=g).to(cuda)).contiguous()
    ref = torch.full((2, 4 + NC, 64), float("nan"), device=cuda)
    _hip.detect_head_into(ref, 0, 1, [f], [f], [wb.to(cuda)], [bb.to(cuda)], [wcd], [bcd], [HEAD_STRIDE], NC)
    y = torch.full((2, 4 + NC, 64), float("nan"), device=cuda)
    with _hook("yolosod_debug_set_conv3x3_head_fuse", 1):
        assert _hip.conv3x3_head_fused(2, 8, 8)
        _hip.conv3x3_head(xd, bd, lambda: prep, lambda: hprep, bcd, 2, NC, HEAD_STRIDE, y, 0)
    assert not _hip.split_range_flag(reset=True)
    assert bool(torch.isnan(y[:, :4]).all()) and bool(torch.isfinite(ref).all())
    assert torch.equal(y[:, 4:], ref[:, 4:]), float((y[:, 4:] - ref[:, 4:]).abs().max())


# ---- f. gemm_f32 on the split products -------------------------------------------------------------------------------

def test_gemm_f32_split_keeps_its_budget(cuda):
    """gemm_f32 with every call forced onto the fp16-split products (yolosod_debug_set_gemm_x2), (M, N, K) =
    (130, 64, 96), K-contiguous B, no activation, operands at 2^-6 with per-column (A) / per-row (B) scales of
    2^-10 .. 2^2:  |C - C64| <= 8 E32 + F, E32 the error of the fp32 matmul on the CPU.

    The floor F, from csrc/gemm_f32.h: the kernel splits sa A and sb B (exact powers of two; x2_sa / x2_sb of the
    launch, 0 meaning 1) and multiplies the accumulators by 1 / (sa sb) before the epilogue. A low term in fp16's
    subnormal range costs 2^-25 on the scaled operand, that is 2^-25 / sa per element of A and 2^-25 / sb per element of
    B, so F_mn = sum_k (2^-25 / sa) |b_nk| + (2^-25 / sb) |a_mk|. yolosod_gemm_f32 (this hook's entry) leaves
    x2_sa = x2_sb = 0, so sa = sb = 1 here and both operands sit on the 2^-25 floor (the A2 / MHA launches that pass a
    weight operand give it 64, which is the conv kernels' 2^-31)."""
    M, N, K = 130, 64, 96
    sa = sbb = 1.0
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g) * S6 * 2.0 ** (torch.rand(1, K, generator=g) * 12 - 10)
    Bm = torch.randn(N, K, generator=g) * S6 * 2.0 ** (torch.rand(N, 1, generator=g) * 12 - 10)
    c64 = A.double() @ Bm.double().t()
    e32 = float(((A @ Bm.t()).double() - c64).abs().max())
    one = torch.ones(M, K, dtype=torch.float64), torch.ones(K, N, dtype=torch.float64)
    fl = (sb.X_FLOOR / sa) * (one[0] @ Bm.double().abs().t()) + (sb.X_FLOOR / sbb) * (A.double().abs() @ one[1])
    lim = 8.0 * e32 + fl
    lib = _hip.load_library()
    _hip.split_range_flag(reset=True)
    lib.yolosod_debug_set_gemm_x2(1)
    try:
        C = _hip.gemm_f32(A.to(cuda).contiguous(), Bm.to(cuda).contiguous(), True)
    finally:
        lib.yolosod_debug_set_gemm_x2(0)
    assert not _hip.split_range_flag(reset=True)
    err = (C.cpu().double() - c64).abs()
    r = float((err / lim).max())
    _log(f"family gemm_f32_x2 ({M}, {N}, {K}) s=2^-6 wide: ratio {r:.3f}, max|err| {float(err.max()):.3g} "
         f"(E32 {e32:.3g})")
    assert r <= 1.0, f"|C - C64| reaches {r:.3f} of 8 E32 + F"
