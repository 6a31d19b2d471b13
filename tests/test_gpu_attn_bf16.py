"""GPU: the bf16 config's SwinBlock, A2_Attn, GEMM, attention and Detect-head kernels in every form they have, against
the fp64 oracle on the same bf16 values, held to the bounds DESIGN.md section 9 states for each kind of operator
(tests/attn_bf16_ref.py): random, structured, all-zero and peaked-softmax inputs, a NaN in the
input, window locality and batch invariance. Every row asserts the route or form it ran through the report hooks
(yolosod_debug_swin_bf16_route / _gemm_bf16_tile / _attention_bf16_form and their last_* twins)."""
import contextlib
import functools

import pytest
import torch

import attn_bf16_ref as br
import attn_ref as ar
from oplib import tol_close
from oracle import ops_ref as R
from yolosod_amd import _hip

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

# NaN share above 0.5 (tests/test_attn_bf16_cpu.py::test_nan_share_and_emulated_mask)
NAN_ROWS = [r for r in br.ROWS if r.shape not in ((1, 512, 9, 9), (1, 128, 12, 40), (1, 256, 12, 24))]


@contextlib.contextmanager
def switched(row):
    """The row's switches set, and put back whatever happens."""
    lib = _hip.load_library()
    undo = []
    try:
        for name, v in row.switches:
            undo.append((name, getattr(lib, f"yolosod_debug_set_{name}")(v)))
        yield
    finally:
        for name, v in undo:
            getattr(lib, f"yolosod_debug_set_{name}")(v)


@functools.lru_cache(maxsize=None)
def _module(op, args, sharp, dev):
    return br.build(op, args, sharp).to(dev)


def run(row, x, cuda, sharp=False):
    """y of the row's bf16 module, with the predicted and the reported route (SwinBlock), attention form and GEMM tiles
    asserted on the way."""
    m = _module(row.op, row.args, sharp, cuda)
    B, C, H, W = x.shape
    heads = br.heads_of(row)
    with switched(row), torch.inference_mode():
        route = None
        if row.op == "SwinBlock":
            route = _hip.swin_bf16_route(B, C, heads, H, W, row.args[2], 2 * C)
            assert route == row.route, (row.id, route)
        n0 = _hip.gemm_bf16_launches()
        y = m(x.to(cuda).to(BF))
        assert y.dtype == BF
        y = y.float().cpu()
        n1 = _hip.gemm_bf16_launches()
        form = br.attn_form(br.attn_len(row), C, heads)
        if row.op == "SwinBlock":
            assert _hip.swin_bf16_last_route() == route, (row.id, _hip.swin_bf16_last_route())
            if route.startswith("fused"):
                assert n1 == n0, (row.id, "a GEMM launch on the fused route")
            else:
                tiles = [_hip.gemm_bf16_tile(mm, nn) for mm, nn in br.swin_gemms(row._replace(shape=tuple(x.shape)))]
                assert {t: n1[t] - n0[t] for t in (64, 128)} == {t: tiles.count(t) for t in (64, 128)}, (row.id, tiles)
                assert _hip.gemm_bf16_last_tile() == tiles[-1]
        else:
            assert sum(n1.values()) - sum(n0.values()) == 3, row.id  # proj, QKV, folded out conv
        if route is None or route.startswith("decomposed"):
            assert _hip.attention_bf16_form(br.attn_len(row), C, heads) == form
            assert _hip.attention_bf16_last_form() == form, (row.id, _hip.attention_bf16_last_form())
    return y


def _check(tag, y, ref):
    mx, mean = br.ratios(y, ref)
    print(f"bf16 {tag}: kernel max {mx:.4f} ({mx / br.BLOCK_MAX:.2f} of the bound) mean {mean:.4f} "
          f"({mean / br.BLOCK_MEAN:.2f})")
    assert mx <= br.BLOCK_MAX and mean <= br.BLOCK_MEAN, (tag, mx, mean)


@pytest.mark.parametrize("row,kind", [pytest.param(r, k, id=f"{r.id}-{k}") for r in br.ROWS for k in br.INPUTS])
def test_parity_in_every_form(row, kind, cuda):
    x, ref = br.case_data(row.op, row.args, row.shape, kind)
    _check(f"{row.id} {kind}", run(row, x, cuda, kind == "sharp"), ref)


@pytest.mark.parametrize("row", NAN_ROWS, ids=lambda r: r.id)
def test_nan_reaches_the_output_as_in_the_oracle(row, cuda):
    """NaN at x[0, 3, 2, 4]: NaN exactly where the fp64 oracle has it, the finite rest inside the bound, and image 1
    bitwise as without the NaN."""
    x0, _ = br.case_data(row.op, row.args, row.shape, "structured")
    x, ref = br.case_data(row.op, row.args, row.shape, "structured", True)
    y = run(row, x, cuda)
    got, want = torch.isnan(y), torch.isnan(ref)
    print(f"bf16 {row.id} nan: mask {int(got.sum())} of oracle's {int(want.sum())}, missing "
          f"{int((want & ~got).sum())}, extra {int((got & ~want).sum())}")
    assert torch.equal(got, want), (row.id, int((want & ~got).sum()), int((got & ~want).sum()))
    assert bool(torch.isfinite(y[~want]).all())
    _check(f"{row.id} nan", y, ref)
    if row.shape[0] > 1:
        assert torch.equal(y[1:], run(row, x0, cuda)[1:])


@pytest.mark.parametrize("row", br.LOCALITY, ids=lambda r: r.id)
def test_swin_windows_do_not_see_each_other(row, cuda):
    """Pixels changed strictly inside one window, two or more pixels from its border (the depthwise 3x3 stays inside),
    change no output bit of any other window."""
    x, _ = br.case_data(row.op, row.args, row.shape, "structured")
    B, C, H, W = row.shape
    img = B - 1
    wy, wx = (1, 0) if H >= 14 else (0, 1)  # a whole 7x7 window that is not the first
    r0, c0 = 7 * wy, 7 * wx
    x2 = x.clone()
    x2[img, :, r0 + 2:r0 + 5, c0 + 2:c0 + 5] += br.rb(torch.randn(C, 3, 3, generator=torch.Generator().manual_seed(5)))
    x2 = br.rb(x2)
    y, y2 = run(row, x, cuda), run(row, x2, cuda)
    others = torch.ones(row.shape, dtype=torch.bool)
    others[img, :, r0:r0 + 7, c0:c0 + 7] = False
    assert torch.equal(y[others], y2[others]), int((y != y2)[others].sum())
    assert not torch.equal(y[~others], y2[~others])


@pytest.mark.parametrize("row", br.ROWS, ids=lambda r: r.id)
def test_batch_invariance(row, cuda):
    """m(x) is bitwise cat(m(x[i:i+1])) at B = 3: the fused kernel's window order and early return, the batched GEMMs."""
    shape = (3,) + row.shape[1:]
    x = br.rb(torch.randn(shape, generator=torch.Generator().manual_seed(17)))
    a = run(row, x, cuda)
    b = torch.cat([run(row, x[i:i + 1], cuda) for i in range(3)])
    assert torch.equal(a, b), float((a - b).abs().max())


def test_a2_refuses_an_unsupported_sequence_before_any_launch(cuda):
    """hd 128 with L = 200: no attention instance fits LDS; the refusal comes ahead of the proj GEMM."""
    row = br.A2_REFUSED
    assert _hip.attention_bf16_form(br.attn_len(row), row.shape[1], br.heads_of(row)) is None
    m = _module(row.op, row.args, False, cuda)
    x = br.make_input(row.op, row.args, row.shape, "randn").to(cuda).to(BF)
    n0, f0 = _hip.gemm_bf16_launches(), _hip.attention_bf16_last_form()
    with pytest.raises(RuntimeError, match="unsupported"), torch.inference_mode():
        m(x)
    assert _hip.gemm_bf16_launches() == n0 and _hip.attention_bf16_last_form() == f0


# ---- the 128x128 tile ----------------------------------------------------------------------------------------------------

GEMM128 = [(4000, 2040, 256, True, None), (4000, 2042, 64, True, None), (4000, 2040, 256, False, None),
           (1000, 1024, 128, False, 8)]


@functools.lru_cache(maxsize=None)
def _gemm_data(M_, N, K, bkc, batch):
    """Operands (bf16 values) and the fp64 product, shared by the epilogue variants."""
    g = torch.Generator().manual_seed(M_ * 7 + N + K)
    nb = () if batch is None else (batch,)
    A = torch.randn(M_, K, generator=g).to(BF)
    B = torch.randn(*nb, *((N, K) if bkc else (K, N)), generator=g).to(BF)
    res = torch.randn(*nb, M_, N, generator=g).to(BF)
    bias = {1: torch.randn(M_, generator=g), 2: torch.randn(N, generator=g)}
    AB = A.double() @ (B.double().transpose(-1, -2) if bkc else B.double())
    return A, B, res, bias, AB


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("act", [1, 2], ids=["silu", "gelu"])
@pytest.mark.parametrize("bias_mode", [1, 2], ids=["biasrow", "biascol"])
@pytest.mark.parametrize("M_,N,K,bkc,batch", GEMM128, ids=lambda v: str(v))
def test_gemm_bf16_tile128(M_, N, K, bkc, batch, bias_mode, act, with_res, cuda):
    """gemm_bf16_kernel<2, 2, 2, 2, ...> (128x128 tiles) against fp64: K- and N-contiguous B, the vector and (N % 4 != 0)
    scalar epilogues, the batched form A2_Attn uses, every bias mode / activation / residual combination."""
    A, B, res, bias, AB = _gemm_data(M_, N, K, bkc, batch)
    assert _hip.gemm_bf16_tile(M_, N, batch or 1) == 128
    n0 = _hip.gemm_bf16_launches()
    C = _hip.gemm_bf16(A.to(cuda), B.to(cuda), bkc, bias[bias_mode].to(cuda), bias_mode, act,
                       res.to(cuda) if with_res else None, batch=batch).double().cpu()
    n1 = _hip.gemm_bf16_launches()
    assert _hip.gemm_bf16_last_tile() == 128 and (n1[64], n1[128]) == (n0[64], n0[128] + 1)
    b = bias[bias_mode].double()
    v = AB + (b[:, None] if bias_mode == 1 else b)
    ref = torch.nn.functional.silu(v) if act == 1 else torch.nn.functional.gelu(v)
    if with_res:
        ref = ref + res.double()
    d = (C - ref).abs()
    lim = br.gemm_limit(ref)
    print(f"bf16 gemm128 {M_}x{N}x{K} bkc={bkc} batch={batch} bias{bias_mode} act{act} res={with_res}: "
          f"{float((d / lim).max()):.3f} of the bound")
    assert bool((d <= lim).all()), f"max|d| {float(d.max()):.3g}, worst ratio {float((d / lim).max()):.2f}"


def test_gemm_bf16_tile64_is_reported(cuda):
    """The other side of the rule, through the same hooks: one tile short of 512."""
    A, B, res, bias, AB = _gemm_data(300, 192, 64, True, None)
    assert _hip.gemm_bf16_tile(300, 192) == 64
    C = _hip.gemm_bf16(A.to(cuda), B.to(cuda), True, bias[2].to(cuda), 2, 1, res.to(cuda)).double().cpu()
    assert _hip.gemm_bf16_last_tile() == 64
    ref = torch.nn.functional.silu(AB + bias[2].double()) + res.double()
    assert bool(((C - ref).abs() <= br.gemm_limit(ref)).all())


@pytest.mark.parametrize("row,kind", [pytest.param(r, k, id=f"{r.id}-{k}") for r in br.TILE128_ROWS
                                      for k in ("randn", "structured")])
def test_swin_with_every_gemm_on_the_128_tile(row, kind, cuda):
    """The decomposed SwinBlock at 33075 padded tokens: all five GEMMs report the 128x128 tile (bias column, GELU,
    residual, and BN + SiLU with the Swin scatter as token pairs at W = 16, single tokens at W = 15)."""
    assert [_hip.gemm_bf16_tile(m, n) for m, n in br.swin_gemms(row)] == [128] * 5
    x = br.make_input(row.op, row.args, row.shape, kind)
    ref = br.oracle_per_image(row.op, row.args, x)
    _check(f"{row.id} {kind}", run(row, x, cuda), ref)


# ---- the attention piece ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sharp", [False, True], ids=["plain", "sharp"])
@pytest.mark.parametrize("L,C,heads", br.ATTN_CASES)
def test_attention_bf16_forms(L, C, heads, sharp, cuda):
    """window_attn_bf16_kernel<HD, NKB> per (head dim, key blocks) against fp64, plain and with q and k sharpened; a NaN
    in one key row of one sequence, inside one head, makes that (sequence, head) NaN and leaves every other output bit
    as without it - for a middle key and for key L - 1, whose copies fill the padding keys."""
    n_seq, hd = br.ATTN_NSEQ, C // heads
    qkv = br.attn_qkv(L, C, heads, sharp)
    form = br.attn_form(L, C, heads)
    assert _hip.attention_bf16_form(L, C, heads) == form
    y = _hip.attention_bf16(qkv.to(cuda).to(BF), n_seq, L, C, heads).float().cpu()
    assert _hip.attention_bf16_last_form() == form
    ref = ar.attention_ref(qkv.double(), n_seq, L, C, heads)
    d = (y.double() - ref).abs()
    lim = br.gemm_limit(ref)
    print(f"bf16 attention L={L} C={C} heads={heads} form {form} sharp={sharp}: {float((d / lim).max()):.3f} of the bound")
    assert bool((d <= lim).all()), f"max|d| {float(d.max()):.3g}, worst ratio {float((d / lim).max()):.2f}"
    for key in (L // 3, L - 1):
        qn = qkv.clone()
        qn[1 * L + key, C + 1 * hd + 3] = float("nan")  # sequence 1, head 1
        yn = _hip.attention_bf16(qn.to(cuda).to(BF), n_seq, L, C, heads).float().cpu()
        want = torch.zeros(n_seq * L, C, dtype=torch.bool)
        want[L:2 * L, hd:2 * hd] = True
        assert torch.equal(torch.isnan(yn), want), (key, int(torch.isnan(yn).sum()), int(want.sum()))
        assert torch.equal(yn[~want], y[~want]), key


def test_attention_bf16_refuses_hd128_beyond_192_keys_without_a_launch(cuda):
    L, C, heads = br.ATTN_REFUSED
    assert _hip.attention_bf16_form(L, C, heads) is None
    qkv = br.attn_qkv(L, C, heads, False).to(cuda).to(BF)
    _hip.attention_bf16(br.attn_qkv(30, 64, 2, False).to(cuda).to(BF), br.ATTN_NSEQ, 30, 64, 2)
    assert _hip.attention_bf16_last_form() == (32, 4)
    with pytest.raises(RuntimeError, match="unsupported"):
        _hip.attention_bf16(qkv, br.ATTN_NSEQ, L, C, heads)
    assert _hip.attention_bf16_last_form() == (32, 4)  # no launch since


# ---- the Detect head on bf16 features -------------------------------------------------------------------------------------

def _head_case(c3, img, peaked):
    """Features rounded to bf16 and fp32 parameters as in test_gpu_ops.py::test_detect_head_fused_vs_oracle; ``peaked``:
    box weights and biases that make each DFL row peak on one bin, as a trained head's do."""
    g = torch.Generator().manual_seed(c3 + img)
    strides, nc, B = [4.0, 8.0, 16.0, 32.0], 10, 2
    fb, fc, wb, bb, wc, bc, maps = [], [], [], [], [], [], []
    for s in strides:
        h = w = int(img // s)
        fb.append(torch.randn(B, 64, h, w, generator=g).to(BF))
        fc.append(torch.randn(B, c3, h, w, generator=g).to(BF))
        wb.append(torch.randn(64, 64, generator=g) * 0.25)
        bb.append(torch.randn(64, generator=g))
        if peaked:
            bb[-1] = bb[-1] + 8.0 * torch.nn.functional.one_hot(torch.randint(0, 16, (4,), generator=g), 16).flatten()
        wc.append(torch.randn(nc, c3, generator=g) * 0.2)
        bc.append(torch.randn(nc, generator=g) - 2.0)
        box = torch.einsum("ok,bkhw->bohw", wb[-1].double(), fb[-1].double()) + bb[-1].double().view(1, -1, 1, 1)
        cls = torch.einsum("ok,bkhw->bohw", wc[-1].double(), fc[-1].double()) + bc[-1].double().view(1, -1, 1, 1)
        maps.append(torch.cat([box, cls], 1))
    return (fb, fc, wb, bb, wc, bc), R.decode_ref(maps, strides, nc), strides, nc


def _head_run(case, x2, cuda):
    args, ref, strides, nc = case
    lib = _hip.load_library()
    prev = lib.yolosod_debug_set_head_x2(x2)
    try:
        assert lib.yolosod_debug_set_head_x2(x2) == x2  # the switch that selects the kernel holds x2
        y = _hip.detect_head(*[[t.to(cuda) for t in ts] for ts in args], strides, nc)
    finally:
        lib.yolosod_debug_set_head_x2(prev)
    assert y.dtype == torch.float32  # the decode stays fp32
    return y.cpu(), ref


@pytest.mark.parametrize("x2", [1, 0], ids=["f16x2_mfma", "fp32_mfma"])
@pytest.mark.parametrize("c3,img", [(64, 256), (128, 256), (64, 200), (128, 200)])
def test_detect_head_bf16_vs_oracle(c3, img, x2, cuda):
    """detect_head_x2_kernel<64, c3, 8, bf16_t> (x2 = 1) and detect_head_lds_kernel<64, c3, 8, bf16_t> (x2 = 0) on bf16
    features against the fp64 oracle on the widened features, at the fp32 head's own bound; 200: a ragged last
    512-pixel block."""
    y, ref = _head_run(_head_case(c3, img, False), x2, cuda)
    ok, err, _ = tol_close(y, ref, 5e-4, 1e-5)
    print(f"bf16 head c3={c3} img={img} x2={x2}: max abs err {err:.3g}")
    assert ok, f"max abs err {err:.3g}"


def _dfl_peak(case):
    """Mean largest DFL probability of the oracle's box logits."""
    (fb, _, wb, bb, _, _), _, _, _ = case
    pk = [torch.softmax((torch.einsum("ok,bkhw->bohw", w.double(), f.double()) + b.double().view(1, -1, 1, 1))
                        .view(f.shape[0], 4, 16, -1), 2).amax(2).flatten() for f, w, b in zip(fb, wb, bb)]
    return float(torch.cat(pk).mean())


@pytest.mark.parametrize("x2", [1, 0], ids=["f16x2_mfma", "fp32_mfma"])
def test_detect_head_bf16_peaked_dfl(x2, cuda):
    """The same with DFL rows peaked on one bin each (mean largest probability above 0.9)."""
    case = _head_case(64, 200, True)
    assert _dfl_peak(case) > 0.9
    y, ref = _head_run(case, x2, cuda)
    ok, err, _ = tol_close(y, ref, 5e-4, 1e-5)
    print(f"bf16 head peaked x2={x2}: max abs err {err:.3g}")
    assert ok, f"max abs err {err:.3g}"


@pytest.fixture(scope="module")
def trained_like_head(tmp_path_factory):
    """The trained-like paper model (tests/trained_like.py) on two noisy scenes of 256 px, on the CPU: the inputs of its
    Detect head's last 1x1 convs rounded to bf16, those convs' fp32 parameters, and the fp64 oracle on them. The mean
    largest DFL probability is 0.30 there (uniform rows: 0.0625)."""
    from oracle.model_ref import REGISTRY
    from trained_like import make_trained_like_checkpoint, noisy_scenes
    from yolosod_amd.nn.checkpoint import attempt_load_one_weight
    path = make_trained_like_checkpoint(tmp_path_factory.mktemp("attn_bf16") / "trained_like.pt")
    cm, _ = attempt_load_one_weight(path, device="cpu", registry=REGISTRY)
    det = cm.model[-1]
    seen = {}
    hooks = [conv[2].register_forward_hook(lambda m, a, o, k=(n, i): seen.__setitem__(k, a[0].detach()))
             for n, cv in (("b", det.cv2), ("c", det.cv3)) for i, conv in enumerate(cv)]
    with torch.inference_mode():
        cm(noisy_scenes(5, 2, 256))
    for h in hooks:
        h.remove()
    strides, nc = [float(s) for s in det.stride], det.nc
    fb = [seen[("b", i)].to(BF) for i in range(det.nl)]
    fc = [seen[("c", i)].to(BF) for i in range(det.nl)]
    wb = [det.cv2[i][2].weight.detach().flatten(1).contiguous() for i in range(det.nl)]
    bb = [det.cv2[i][2].bias.detach().clone() for i in range(det.nl)]
    wc = [det.cv3[i][2].weight.detach().flatten(1).contiguous() for i in range(det.nl)]
    bc = [det.cv3[i][2].bias.detach().clone() for i in range(det.nl)]
    maps = [torch.cat([torch.einsum("ok,bkhw->bohw", wb[i].double(), fb[i].double()) + bb[i].double().view(1, -1, 1, 1),
                       torch.einsum("ok,bkhw->bohw", wc[i].double(), fc[i].double()) + bc[i].double().view(1, -1, 1, 1)],
                      1) for i in range(det.nl)]
    return (fb, fc, wb, bb, wc, bc), R.decode_ref(maps, strides, nc), strides, nc


@pytest.mark.parametrize("x2", [1, 0], ids=["f16x2_mfma", "fp32_mfma"])
def test_detect_head_bf16_trained_like(trained_like_head, x2, cuda):
    """The bf16 head kernels on a trained-like head's own features: unit-variance activations, peaked DFL rows."""
    assert _dfl_peak(trained_like_head) > 0.25
    y, ref = _head_run(trained_like_head, x2, cuda)
    ok, err, _ = tol_close(y, ref, 5e-4, 1e-5)
    print(f"bf16 head trained-like x2={x2}: max abs err {err:.3g}, DFL peak {_dfl_peak(trained_like_head):.2f}")
    assert ok, f"max abs err {err:.3g}"
