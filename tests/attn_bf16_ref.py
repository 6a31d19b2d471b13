"""Test helper for the bf16 config's token-mixing kernels (csrc/swin_fused_bf16.hip, csrc/transformer_bf16.hip,
csrc/gemm_bf16.h). No GPU calls.

* ``SWIN_ROWS`` / ``A2_ROWS`` / ``TILE128_ROWS``: every (operator, kernel form) under test with the switches that select
  it and the route the library must report (``_hip.SWIN_BF16_ROUTES``); DESIGN.md section 33 has the table.
* ``make_input``: attn_ref's ``randn`` / ``structured`` / ``zeros`` inputs (``sharp``: structured, the module sharpened
  with ``attn_ref.sharpen``), rounded to bf16.
* ``oracle``: oracle.model_ref.OP_CLASSES in fp64 on the bf16-rounded parameters and input (what
  tests/test_gpu_bf16.py::_bf16_oracle does); ``ratios``: max|d| / max|ref| and mean|d| / mean|ref| over the elements
  finite in the oracle, the two figures of the block bound of DESIGN.md section 9 (BLOCK_MAX, BLOCK_MEAN).
* ``emulate``: SwinBlock and A2_Attn on the CPU in fp32 with a round-to-bf16 at each storage point of section 9, and
  ``MUTANTS``: bugs these kernels could have. ``attention_emul``: the attention piece with P rounded to bf16.

tests/test_attn_bf16_cpu.py shows that the emulation keeps the bounds and that every mutant breaks them;
tests/test_gpu_attn_bf16.py holds the kernels to them."""
from __future__ import annotations

import functools
import math

import torch
import torch.nn.functional as F

import attn_ref as ar
from attn_ref import Row
from oracle import ops_ref as R
from oracle.model_ref import OP_CLASSES
from yolosod_amd.nn import modules as M

BF = torch.bfloat16
BLOCK_MAX, BLOCK_MEAN = 2.5e-2, 1e-2  # tests/test_gpu_bf16.py: BF16_BLOCK_REL and the mean bound
SHARPEN_QK = 2.0  # the attention piece: q and k scaled by this (scores x 4); test_attn_bf16_cpu.py shows the emulation fits

TOK2 = (("swin_tokln", 0),)
SWIN_ROWS = [
    Row("SwinBlock", (64, 2, 7), (2, 64, 9, 56), (), "fused_chunked", "<64, 2>, all eight hoff, cropped rows"),
    Row("SwinBlock", (64, 2, 7), (2, 64, 20, 13), (), "fused_2byte", "<64, 2>, cropped both ways"),
    Row("SwinBlock", (128, 4, 7), (1, 128, 9, 56), (), "fused_chunked", "<128, 4>"),
    Row("SwinBlock", (128, 4, 7), (1, 128, 9, 13), (), "fused_2byte", "<128, 4>"),
    Row("SwinBlock", (128, 2, 7), (1, 128, 16, 24), (), "fused_chunked", "<128, 2>"),
    Row("SwinBlock", (128, 2, 7), (1, 128, 9, 13), (), "fused_2byte", "<128, 2>"),
    Row("SwinBlock", (64, 2, 7), (2, 64, 6, 5), (), "decomposed_tok2", "by shape: one 6x5 window, L = 30"),
    Row("SwinBlock", (256, 4, 7), (1, 256, 14, 9), (), "decomposed_tok2", "odd W: single-token scatter"),
    Row("SwinBlock", (256, 4, 7), (1, 256, 9, 16), (), "decomposed_tokln", "pair scatter, tokens + LN1 pass"),
    Row("SwinBlock", (256, 4, 7), (1, 256, 9, 16), TOK2, "decomposed_tok2", "pair scatter, two-kernel token path"),
    Row("SwinBlock", (512, 4, 7), (1, 512, 9, 9), (), "decomposed_tok2", "hd 128"),
    Row("SwinBlock", (256, 8, 7), (1, 256, 9, 16), (), "decomposed_tokln", "hd 32"),
]
A2_ROWS = [
    Row("A2_Attn", (192, None, 4, 3), (2, 192, 10, 20), (), None, "hd 64, L = 80"),
    Row("A2_Attn", (512, None, 8, 8), (2, 512, 20, 20), (), None, "hd 64, L = 160"),
    Row("A2_Attn", (128, None, 8, 4), (1, 128, 12, 40), (), None, "hd 32, L = 320, overlapping pool bins"),
    Row("A2_Attn", (256, None, 8, 2), (1, 256, 12, 24), (), None, "hd 128, L = 192"),
]
A2_REFUSED = Row("A2_Attn", (256, None, 8, 2), (1, 256, 16, 25), (), None, "hd 128, L = 200: no instance fits LDS")
ROWS = SWIN_ROWS + A2_ROWS
# all five GEMMs of the decomposed SwinBlock on the 128x128 tile (33075 padded tokens), pair and single-token scatter
TILE128_ROWS = [
    Row("SwinBlock", (256, 4, 7), (75, 256, 16, 16), (), "decomposed_tokln", "128x128 tiles, pair scatter"),
    Row("SwinBlock", (256, 4, 7), (75, 256, 16, 15), (), "decomposed_tok2", "128x128 tiles, single-token scatter"),
]
INPUTS = ar.INPUTS
LOCALITY = [SWIN_ROWS[0], SWIN_ROWS[1], SWIN_ROWS[7]]
MODULE_SHAPES = list(dict.fromkeys((r.op, r.args, r.shape) for r in ROWS))


def heads_of(row):
    return row.args[1] if row.op == "SwinBlock" else row.args[3]


def attn_len(row):
    """Tokens per attention sequence of the row."""
    B, C, H, W = row.shape
    if row.op == "A2_Attn":
        return row.args[2] * W
    ws = row.args[2]
    return H * W if (H <= ws and W <= ws) else min(ws, H) * min(ws, W)


def swin_gemms(row):
    """(M, N) of the five GEMMs of the decomposed bf16 SwinBlock, in launch order (QKV, out-proj, MLP1, MLP2, pw)."""
    B, C, H, W = row.shape
    ws = row.args[2]
    wh, ww = (H, W) if (H <= ws and W <= ws) else (min(ws, H), min(ws, W))
    ntok = B * (-(-H // wh) * wh) * (-(-W // ww) * ww)
    return [(ntok, 3 * C), (ntok, C), (ntok, 2 * C), (ntok, C), (C, ntok)]


# ---- inputs, modules, the oracle ----------------------------------------------------------------------------------------

def rb(t):
    """Round to bf16 (to nearest even), back in fp32."""
    return t.to(BF).float()


def make_input(op, args, shape, kind):
    return rb(ar.make_input(op, args, shape, kind))


def build(op, args, sharp=False, classes=None):
    """The module with recipe parameters rounded to bf16 (as ``model.to(torch.bfloat16)`` leaves them), still bf16."""
    return ar.build(op, args, sharp, classes).to(BF)


def oracle(op, args, x, sharp=False):
    m = build(op, args, sharp, OP_CLASSES).double()
    with torch.inference_mode():
        return m(x.double())


@functools.lru_cache(maxsize=None)
def case_data(op, args, shape, kind, nan=False):
    """(x, ref64) of a case, computed once and shared; callers must not modify them."""
    x = make_input(op, args, shape, kind)
    if nan:
        x = ar.with_nan(x)
    return x, oracle(op, args, x, kind == "sharp")


def oracle_per_image(op, args, x, sharp=False):
    """The oracle image by image (it is batch-independent): less memory at large B."""
    m = build(op, args, sharp, OP_CLASSES).double()
    with torch.inference_mode():
        return torch.cat([m(x[i:i + 1].double()) for i in range(x.shape[0])])


def ratios(y, ref64):
    """(max|d| / max|ref|, mean|d| / mean|ref|) over the elements finite in the oracle; (inf, inf) when y's NaN mask is
    not the oracle's."""
    y = y.double()
    if not torch.equal(torch.isnan(y), torch.isnan(ref64)):
        return float("inf"), float("inf")
    ok = torch.isfinite(ref64)
    if not bool(ok.any()):
        return 0.0, 0.0
    d, r = (y - ref64)[ok].abs(), ref64[ok].abs()
    if float(r.max()) == 0.0:
        return (0.0, 0.0) if float(d.max()) == 0.0 else (float("inf"), float("inf"))
    return float(d.max() / r.max()), float(d.mean() / r.mean())


def within(y, ref64):
    mx, mean = ratios(y, ref64)
    return mx <= BLOCK_MAX and mean <= BLOCK_MEAN


# ---- the emulation: fp32 arithmetic, bf16 at the storage points of DESIGN.md section 9 ---------------------------------

SWIN_MUTANTS = ("halo_left_zero", "pad_tokens_conv", "last_key_masked", "vt_pad_nan", "scale_sqrt_c")
A2_MUTANTS = ("last_key_masked", "vt_pad_nan", "scale_sqrt_c", "pool_bin_shift")
MUTANTS = {"SwinBlock": SWIN_MUTANTS, "A2_Attn": A2_MUTANTS}


def applies(mutant, row):
    """Whether the mutant changes anything on the row's shape: the left halo needs a second window column, the pad
    tokens a cropped window, the V^T padding keys a sequence that is no multiple of 32 keys."""
    B, C, H, W = row.shape
    L = attn_len(row)
    if mutant == "halo_left_zero":
        return L == 49 and W > 7
    if mutant == "pad_tokens_conv":
        return L != H * W and (H % 7 != 0 or W % 7 != 0)
    if mutant == "vt_pad_nan":
        return L % 32 != 0
    return True


def _mha_emul(u, in_w, in_b, heads, mutant):
    """u [n_seq, L, C] (bf16 values) -> P.V [n_seq, L, C]; storage points: QKV, P, P.V."""
    n, L, C = u.shape
    hd = C // heads
    qkv = rb(u @ in_w.t() + in_b)
    q, k, v = (t.reshape(n, L, heads, hd).transpose(1, 2) for t in qkv.split(C, dim=-1))
    s = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(C if mutant == "scale_sqrt_c" else hd))
    if mutant == "last_key_masked":
        s[..., L - 1] = float("-inf")
    p = rb(torch.softmax(s, dim=-1))
    o = p @ v
    if mutant == "vt_pad_nan" and L % 32 != 0:
        # the padding keys meet P = 0 exactly; a V^T tile that is not zeroed there holds whatever the LDS held
        o = o + torch.zeros(()) * float("nan")
    return rb(o).transpose(1, 2).reshape(n, L, C)


def swin_emul(m, x, mutant=None):
    """m: the bf16-rounded SwinBlock widened to fp32. Storage points: depthwise conv, LN1, QKV, P, P.V, out-proj +
    residual, LN2, GELU(MLP1), MLP2 + residual, output."""
    wa, at, bn = m.window_attn, m.window_attn.attn, m.bn
    B, C, H, W = x.shape
    ws = wa.window_size
    t = F.conv2d(x, m.dw.weight, padding=1, groups=C)
    if mutant == "halo_left_zero" and H * W > ws * ws:
        for c0 in range(ws, W, ws):  # first column of every window with wx > 0: its left neighbour read as zero
            xz = x.clone()
            xz[..., c0 - 1] = 0.0
            t[..., c0] = F.conv2d(xz, m.dw.weight, padding=1, groups=C)[..., c0]
    t = rb(t)
    if mutant == "pad_tokens_conv" and not (H <= ws and W <= ws):
        Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
        t = rb(F.conv2d(F.pad(x, (0, Wp - W, 0, Hp - H)), m.dw.weight, padding=1, groups=C))
    win, size, wsz = R.window_partition_ref(t, ws)
    u = rb(F.layer_norm(win, (C,), wa.norm1.weight, wa.norm1.bias, wa.norm1.eps))
    o = _mha_emul(u, at.in_proj_weight, at.in_proj_bias, at.num_heads, mutant)
    win = rb(win + (o @ at.out_proj.weight.t() + at.out_proj.bias))
    u = rb(F.layer_norm(win, (C,), wa.norm2.weight, wa.norm2.bias, wa.norm2.eps))
    hmid = rb(F.gelu(u @ wa.mlp[0].weight.t() + wa.mlp[0].bias))
    win = rb(win + (hmid @ wa.mlp[2].weight.t() + wa.mlp[2].bias))
    y = R.window_reverse_ref(win, size, wsz)[:, :, :H, :W]
    y = F.conv2d(y, m.pw.weight)
    y = R._bn_eval(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
    return rb(x + F.silu(y))


def _pool_rows(xp, A, shift):
    """adaptive_avg_pool2d(xp, (A, W)) with every bin moved down by ``shift`` rows (clamped to the map)."""
    H = xp.shape[2]
    rows = []
    for i in range(A):
        lo, hi = (i * H) // A, -(-((i + 1) * H) // A)
        lo, hi = min(lo + shift, H - 1), min(hi + shift, H)
        rows.append(xp[:, :, lo:hi].mean(2))
    return torch.stack(rows, 2)


def a2_emul(m, x, mutant=None):
    """m: the bf16 A2_Attn (its fold of the MHA out-projection into the output conv is made from the bf16 parameters and
    stored in bf16, as the product's). Storage points: proj + SiLU, pooled tokens, LN, QKV, P, P.V, folded out conv,
    output."""
    B, C, H, W = x.shape
    A = m.num_areas
    pw, pb = (t.float() for t in M.conv_weight_bias(m.proj))
    fw, fb = (t.float() for t in m._fused_out())
    ln, at = m.layer_norm, m.attention
    xp = rb(F.silu(F.conv2d(x, pw.reshape(C, C, 1, 1), pb)))
    seq = rb(_pool_rows(xp, A, 1 if mutant == "pool_bin_shift" else 0)).flatten(2).transpose(1, 2)
    s = rb(F.layer_norm(seq, (C,), ln.weight.float(), ln.bias.float(), ln.eps))
    o = _mha_emul(s, at.in_proj_weight.float(), at.in_proj_bias.float(), m.num_heads, mutant)
    z = rb(o @ fw.flatten(1).t()).transpose(1, 2).reshape(B, C, A, W)
    up = F.interpolate(z, size=(H, W), mode="bilinear", align_corners=False)
    return rb(F.silu(up + fb[None, :, None, None]) + x)


def emulate(op, args, x, sharp=False, mutant=None):
    m = build(op, args, sharp)
    with torch.inference_mode():
        if op == "SwinBlock":
            return swin_emul(m.float(), x, mutant)
        return a2_emul(m, x, mutant)


# ---- the attention piece -------------------------------------------------------------------------------------------

ATTN_CASES = [(30, 64, 2), (200, 128, 4), (320, 128, 4),                                                   # hd 32
              (64, 128, 2), (65, 128, 2), (128, 256, 4), (192, 256, 4), (250, 128, 2), (320, 512, 8),      # hd 64
              (81, 256, 2), (128, 512, 4), (192, 256, 2)]                                                   # hd 128
ATTN_REFUSED = (193, 256, 2)
ATTN_NSEQ = 2


def attn_form(L, C, heads):
    """(head dim, key blocks of the instance): the smallest compiled count >= the sequence's 32-key steps."""
    nkb = -(-L // 32) * 2
    return C // heads, next(n for n in (4, 6, 8, 10, 12, 16, 20) if n >= nkb)


def attn_qkv(L, C, heads, sharp):
    """The packed qkv of test_gpu_bf16.py::test_attention_bf16 (1.5 randn), q and k scaled when ``sharp``; bf16
    values in fp32."""
    qkv = torch.randn(ATTN_NSEQ * L, 3 * C, generator=torch.Generator().manual_seed(L * 13 + C)) * 1.5
    if sharp:
        qkv[:, :2 * C] *= SHARPEN_QK
    return rb(qkv)


def attention_emul(qkv, n_seq, L, C, heads):
    hd = C // heads
    q, k, v = qkv.view(n_seq, L, 3, heads, hd).permute(2, 0, 3, 1, 4)
    p = rb(torch.softmax(q @ k.transpose(-1, -2) / hd ** 0.5, -1))
    return rb(p @ v).transpose(1, 2).reshape(n_seq * L, C)


def gemm_limit(ref):
    """The GEMM / attention bound of DESIGN.md section 9: 2^-7 |ref| + 2^-8 max|ref|."""
    return 2.0 ** -7 * ref.abs() + 2.0 ** -8 * float(ref.abs().max())
