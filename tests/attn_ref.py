"""Test helper for the token-mixing operators of the neck (SwinBlock, A2_Attn, MambaBlock: csrc/transformer.hip,
csrc/swin_x3.hip, csrc/swin_fused.hip, csrc/swin_wide.hip, csrc/a2_fused.hip, csrc/mamba_glu.hip) and the pieces under
them (layernorm, attention). No GPU calls.

* ``ROWS``: every (operator, route) under test with the switches that select it and the route SwinBlock must report
  (DESIGN.md section 30 has the table).
* ``structured`` / ``zeros`` / ``with_nan`` / ``with_inf``: the inputs; ``sharpen`` peaks the softmax rows.
* ``oracle`` / ``bound`` / ``worst_ratio``: the fp64 oracle (oracle.model_ref.OP_CLASSES), the same module in fp32 on the
  CPU, and the bound   |y - ref64| <= K E32 + 2^-23 |ref64|   with E32 = max |ref32 - ref64|.
* ``emulate``: SwinBlock and A2_Attn in fp32 on the CPU with every matrix product as the fp16 two-term split
  ah.bh + ah.bl + al.bh (tests/split_budget.py), and mutants that drop one low-term product of one matrix product.

tests/test_attn_family_cpu.py shows that the emulation keeps the bound and that every mutant breaks it;
tests/test_gpu_attn_family.py holds the kernels to it."""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import torch
import torch.nn.functional as F

import recipes
import split_budget as sb
from oplib import build_module
from oracle import ops_ref as R
from oracle.model_ref import OP_CLASSES
from yolosod_amd.nn import modules as M

# The next power of two above the worst ratio max|y - ref64| / E32 of the emulation (CPU: 2.57) and of the kernels
# (MI355X: 2.97), both listed in DESIGN.md section 30; 8 is the ceiling (the project's ratio for its own
# fp32-accumulation kernels against a library op, tests/split_budget.py).
K = 4.0

OFFSET, OUTLIER = 12.5, 6.25  # the values tests/channel_ref.py ended on
SPECIAL_AT = (0, 3, 2, 4)     # where with_nan / with_inf put their value
SHARPEN = 3.0


class Row(NamedTuple):
    op: str
    args: tuple
    shape: tuple
    switches: tuple   # ((setter name without the yolosod_debug_set_ prefix, value), ...), restored by the tests
    route: str | None  # SwinBlock: the route the library must report (_hip.SWIN_ROUTES)
    note: str

    @property
    def id(self):
        a = "-".join("x" if v is None else str(v) for v in self.args)
        sw = "".join(f"-{k}{v}" for k, v in self.switches)
        return f"{self.op}-{a}-{'x'.join(map(str, self.shape))}{sw}"

    @property
    def module_key(self):
        return (self.op, self.args)


X3_OFF = (("swin_x3", 0),)
GEMM_ONLY = (("swin_fused", 0), ("swin_x3", 0))
SWIN_ROWS = [
    Row("SwinBlock", (64, 2, 7), (2, 64, 20, 13), (), "split_fused", "swin_x3_kernel<64, 2>, cropped windows"),
    Row("SwinBlock", (256, 4, 7), (1, 256, 14, 9), (), "split_fused", "swin_wx_kernel, cropped windows"),
    Row("SwinBlock", (64, 2, 7), (2, 64, 20, 13), X3_OFF, "exact_fused", "swin_fused_kernel<64, 2, true>"),
    Row("SwinBlock", (64, 4, 7), (1, 64, 14, 9), X3_OFF, "exact_fused", "<64, 4, true>"),
    Row("SwinBlock", (128, 2, 7), (1, 128, 9, 16), X3_OFF, "exact_fused", "<128, 2, true>"),
    Row("SwinBlock", (128, 4, 7), (1, 128, 9, 16), X3_OFF, "exact_fused", "<128, 4, true>"),
    Row("SwinBlock", (64, 2, 7), (2, 64, 6, 5), (), "exact_fused", "<64, 2, false>: one 6x5 window per image"),
    Row("SwinBlock", (64, 4, 7), (2, 64, 6, 5), (), "exact_fused", "<64, 4, false>"),
    Row("SwinBlock", (128, 2, 7), (2, 128, 6, 5), (), "exact_fused", "<128, 2, false>"),
    Row("SwinBlock", (128, 4, 7), (2, 128, 6, 5), (), "exact_fused", "<128, 4, false>"),
    Row("SwinBlock", (128, 4, 7), (1, 128, 5, 16), (), "exact_fused", "<128, 4, false>: 5x7 windows, cropped"),
    Row("SwinBlock", (256, 4, 7), (1, 256, 14, 9), X3_OFF, "exact_wide", "swin_wide_kernel"),
    Row("SwinBlock", (256, 4, 7), (2, 256, 6, 5), (), "decomposed", "by shape: hd 64, whole-sequence attention"),
    Row("SwinBlock", (256, 4, 7), (1, 256, 5, 16), (), "decomposed", "by shape: hd 64, 5x7 windows"),
    Row("SwinBlock", (96, 3, 7), (1, 96, 9, 16), (), "decomposed", "by shape: hd 32, 32-channel partition tail"),
    Row("SwinBlock", (512, 4, 7), (1, 512, 9, 9), (), "decomposed", "by shape: hd 128"),
    Row("SwinBlock", (64, 2, 7), (2, 64, 20, 13), GEMM_ONLY, "decomposed", "by switch"),
    Row("SwinBlock", (256, 4, 7), (1, 256, 14, 9), GEMM_ONLY, "decomposed", "by switch"),
]
A2_MODULES = [((192, None, 4, 3), (2, 192, 10, 20), "4 areas of 3 rows, hd 64"),
              ((512, None, 8, 8), (2, 512, 20, 20), "the model's L12"),
              ((64, None, 8, 8), (2, 64, 4, 8), "hd 8: never fused")]
A2_ROWS = [Row("A2_Attn", a, s, (("a2_fused", f), ("a2_x2", x2)), None, n)
           for a, s, n in A2_MODULES for f in (0, 1) for x2 in (0, 1)]
MAMBA_ROWS = [Row("MambaBlock", (64, 64, 2), (2, 64, 15, 13), (), None, "odd map, reduction 2"),
              Row("MambaBlock", (32, 64, 1), (2, 32, 10, 12), (), None, "no reduction"),
              Row("MambaBlock", (64, 32, 3), (1, 64, 14, 17), (), None, "reduction 3")]
ROWS = SWIN_ROWS + A2_ROWS + MAMBA_ROWS
INPUTS = ("randn", "structured", "zeros", "sharp")  # sharp: structured with sharpen(m), SwinBlock and A2_Attn only
# rows that run the same (module, input) on two or three routes
CROSS = [[r for r in ROWS if r.module_key == k and r.shape == s]
         for k, s in dict.fromkeys((r.module_key, r.shape) for r in ROWS)]
CROSS = [g for g in CROSS if len(g) > 1]
LOCALITY = [r for r in SWIN_ROWS if r.shape in ((2, 64, 20, 13), (1, 256, 14, 9))]
# one (module, shape) per distinct data set of the CPU tests
MODULE_SHAPES = list(dict.fromkeys((r.op, r.args, r.shape) for r in ROWS))


def inputs_of(row):
    return INPUTS if row.op != "MambaBlock" else INPUTS[:3]


# ---- inputs ---------------------------------------------------------------------------------------------------------

def structured(shape, seed):
    """randn [B, C, H, W] plus: every fifth plane + OFFSET; a 3x4 pixel block + OFFSET in all channels (a large
    LayerNorm mean); +OUTLIER at pixel (0, 0) and -OUTLIER at (H-1, W-1), where the zero pad meets the 3x3 halo; one
    full row constant."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    x[:, 0::5] += OFFSET
    r0, c0 = min(H // 3, max(H - 3, 0)), min(W // 3, max(W - 4, 0))
    x[:, :, r0:r0 + 3, c0:c0 + 4] += OFFSET
    x[:, :, 0, 0] = OUTLIER
    x[:, :, H - 1, W - 1] = -OUTLIER
    x[:, :, (2 * H) // 3, :] = 0.75
    return x.contiguous()


def zeros(shape):
    return torch.zeros(shape)


def with_nan(x):
    x = x.clone()
    x[SPECIAL_AT] = float("nan")
    return x


def with_inf(x):
    x = x.clone()
    x[SPECIAL_AT] = float("inf")
    return x


# ---- modules and the oracle -------------------------------------------------------------------------------------------

def _mha(m):
    return m.window_attn.attn if isinstance(m, M.SwinBlock) else m.attention


def sharpen(m):
    """Scale the q and k rows of in_proj_weight by SHARPEN, in place (the scores grow ninefold): on the structured
    2x64x20x13 SwinBlock case the mean of the largest attention probability per row goes from 0.14 to 0.67, zero-pad
    tokens of the cropped windows included."""
    at = _mha(m)
    with torch.no_grad():
        at.in_proj_weight[:2 * at.embed_dim].mul_(SHARPEN)
    return m


def seed_of(op, args):
    return recipes.seed_of(f"{op}-{'-'.join(map(str, args))}")


def build(op, args, sharp=False, classes=None):
    """The product module (or, with classes=OP_CLASSES, the oracle's) with recipe parameters, on the CPU in fp32."""
    m, _ = build_module(op, args, args[0], seed_of(op, args), classes)
    return sharpen(m) if sharp else m


def make_input(op, args, shape, kind):
    """kind: randn / structured / zeros / sharp (= structured; the module is sharpened)."""
    seed = seed_of(op, args) + 1 + 1000 * shape[2] + shape[3]
    if kind == "zeros":
        return zeros(shape)
    if kind == "randn":
        return torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    return structured(shape, seed)


class Ref(NamedTuple):
    ref64: torch.Tensor
    nonfinite32: torch.Tensor  # the fp32 oracle's non-finite mask
    e32: float


def oracle(op, args, x, sharp=False):
    """ref64, the fp32 oracle's non-finite mask, and E32 = max |ref32 - ref64| over the elements finite in both."""
    m = build(op, args, sharp, OP_CLASSES)
    with torch.inference_mode():
        ref32 = m(x).double()
        ref64 = m.double()(x.double())
    ok = torch.isfinite(ref32) & torch.isfinite(ref64)
    e32 = float((ref32 - ref64)[ok].abs().max()) if bool(ok.any()) else 0.0
    return Ref(ref64, ~torch.isfinite(ref32), e32)


@functools.lru_cache(maxsize=None)
def case_data(op, args, shape, kind, special=None):
    """(x, Ref) of a case, computed once and shared; callers must not modify them. special: None / "nan" / "inf" at
    x[SPECIAL_AT]."""
    x = make_input(op, args, shape, kind)
    if special:
        x = with_nan(x) if special == "nan" else with_inf(x)
    return x, oracle(op, args, x, kind == "sharp")


def bound(ref64, e32, k=K):
    return k * e32 + 2.0 ** -23 * ref64.abs()


def worst_ratio(y, ref64, e32, k=K, nonfinite=None):
    """max |y - ref64| / bound over the finite elements of the reference; inf when the NaN masks differ (with
    ``nonfinite``: when y's non-finite mask is not that one)."""
    y = y.double()
    if nonfinite is None:
        same = torch.equal(torch.isnan(y), torch.isnan(ref64))
    else:
        same = torch.equal(~torch.isfinite(y), nonfinite)
    if not same:
        return float("inf")
    ok = torch.isfinite(ref64) if nonfinite is None else ~nonfinite & torch.isfinite(ref64)
    if not bool(ok.any()):
        return 0.0
    r = ((y - ref64).abs() / bound(ref64, e32, k))[ok].max()
    return float("inf") if torch.isnan(r) else float(r)


def e32_ratio(y, ref64, e32):
    """max |y - ref64| / E32 over the finite elements of the reference: the figure K is chosen from."""
    ok = torch.isfinite(ref64)
    return float((y.double() - ref64)[ok].abs().max()) / e32


def nan_share(ref64):
    return float(torch.isnan(ref64).double().mean())


# ---- the pieces -----------------------------------------------------------------------------------------------------

def attention_ref(qkv, n_seq, L, C, heads):
    """softmax(q k^T / sqrt(hd)) v per (sequence, head) on packed qkv [n_seq * L, 3C], in qkv's dtype (the restatement of
    tests/test_gpu_ops.py::test_attention)."""
    hd = C // heads
    q, k, v = qkv.view(n_seq, L, 3, heads, hd).permute(2, 0, 3, 1, 4)
    p = torch.softmax(q @ k.transpose(-1, -2) / hd ** 0.5, -1)
    return (p @ v).transpose(1, 2).reshape(n_seq * L, C)


# ---- fp32 emulation with split products ------------------------------------------------------------------------------

TERMS = ("al_bh", "ah_bl")
SWIN_PRODUCTS = ("in_proj", "qk", "pv", "out_proj", "mlp1", "mlp2", "pw")
A2_PRODUCTS = ("proj", "in_proj", "qk", "pv", "out")
MUTANTS = {"SwinBlock": [(p, t) for p in SWIN_PRODUCTS for t in TERMS],
           "A2_Attn": [(p, t) for p in A2_PRODUCTS for t in TERMS]}


class _Mm:
    """a @ b as ah.bh + ah.bl + al.bh with h = fp16(v), l = fp16(v - h), summed smallest first in fp32; the mutant
    (product, term) drops that term of that product. Weights are split as 64 W (csrc/split_conv.h)."""

    def __init__(self, mutant):
        self.mutant = mutant

    def __call__(self, name, a, b):
        ah, al = sb._split(a)
        bh, bl = sb._split(b)
        drop = self.mutant[1] if self.mutant and self.mutant[0] == name else None
        acc = torch.zeros((), dtype=torch.float32)
        if drop != "al_bh":
            acc = acc + al @ bh
        if drop != "ah_bl":
            acc = acc + ah @ bl
        return acc + ah @ bh

    def lin(self, name, a, w):
        """a @ w^T with the weight split as 64 W."""
        return self(name, a, (w * sb.WSC).t()) * (1.0 / sb.WSC)


def _mha_emul(mm, u, in_w, in_b, heads):
    B, L, C = u.shape
    hd = C // heads
    qkv = mm.lin("in_proj", u, in_w) + in_b
    q, k, v = qkv.split(C, dim=-1)
    q = q.reshape(B, L, heads, hd).transpose(1, 2) * (1.0 / math.sqrt(hd))
    k = k.reshape(B, L, heads, hd).transpose(1, 2)
    v = v.reshape(B, L, heads, hd).transpose(1, 2)
    p = torch.softmax(mm("qk", q, k.transpose(-1, -2)), dim=-1)
    return mm("pv", p, v).transpose(1, 2).reshape(B, L, C)


def swin_emul(m, x, mutant=None):
    mm = _Mm(mutant)
    wa, at, bn = m.window_attn, m.window_attn.attn, m.bn
    B, C, H, W = x.shape
    t = F.conv2d(x, m.dw.weight, padding=1, groups=C)
    win, size, wsz = R.window_partition_ref(t, wa.window_size)
    u = F.layer_norm(win, (C,), wa.norm1.weight, wa.norm1.bias, wa.norm1.eps)
    o = _mha_emul(mm, u, at.in_proj_weight, at.in_proj_bias, at.num_heads)
    win = win + (mm.lin("out_proj", o, at.out_proj.weight) + at.out_proj.bias)
    u = F.layer_norm(win, (C,), wa.norm2.weight, wa.norm2.bias, wa.norm2.eps)
    hmid = F.gelu(mm.lin("mlp1", u, wa.mlp[0].weight) + wa.mlp[0].bias)
    win = win + (mm.lin("mlp2", hmid, wa.mlp[2].weight) + wa.mlp[2].bias)
    y = R.window_reverse_ref(win, size, wsz)[:, :, :H, :W]
    y = mm.lin("pw", y.permute(0, 2, 3, 1), m.pw.weight.flatten(1)).permute(0, 3, 1, 2)
    y = R._bn_eval(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
    return x + F.silu(y)


def a2_emul(m, x, mutant=None):
    mm = _Mm(mutant)
    B, C, H, W = x.shape
    A = m.num_areas
    pw, pb = M.conv_weight_bias(m.proj)
    fw, fb = m._fused_out()  # the MHA out-projection folded into the output conv, as the product runs it
    xp = F.silu(mm.lin("proj", x.permute(0, 2, 3, 1), pw.flatten(1)) + pb).permute(0, 3, 1, 2)
    seq = F.adaptive_avg_pool2d(xp, (A, W)).flatten(2).transpose(1, 2)
    s = F.layer_norm(seq, (C,), m.layer_norm.weight, m.layer_norm.bias, m.layer_norm.eps)
    o = _mha_emul(mm, s, m.attention.in_proj_weight, m.attention.in_proj_bias, m.num_heads)
    z = mm.lin("out", o, fw.flatten(1))                      # the bilinear upsample commutes with the 1x1 conv
    z = z.transpose(1, 2).reshape(B, C, A, W)
    up = F.interpolate(z, size=(H, W), mode="bilinear", align_corners=False)
    return F.silu(up + fb[None, :, None, None]) + x


def emulate(op, args, x, sharp=False, mutant=None):
    """y of ``op`` in fp32 with split matrix products (recipe parameters)."""
    m = build(op, args, sharp)
    with torch.inference_mode():
        return (swin_emul if op == "SwinBlock" else a2_emul)(m, x, mutant)
