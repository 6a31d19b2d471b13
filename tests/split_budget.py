"""Test helper: the a-priori error budget of the fp16 two-term split conv kernels (csrc/common.h, csrc/split_conv.h,
DESIGN.md section 4) and a CPU emulation of their arithmetic, with mutants that lose one term each. No GPU calls.

The split writes v = h + l with h = fp16(v), l = fp16(v - h). While l is a normal fp16 number |v - h - l| <= 2^-22 |v|;
once l falls into fp16's subnormal range (|v| < 2^-3 for an activation) its spacing is 2^-24, so the representation
costs an absolute 2^-25 per element. The weights are split as 64 W, which moves their floor to 2^-25 / 64 = 2^-31.
Per output element the floor is therefore

    F = sum_k 2^-25 |w_nk| + 2^-31 |x_k|

and the budget is  lim = 8 E32 + 1.1 F:  E32 the error of a plain fp32 conv (torch on the CPU) against fp64, 8 the
project's ratio of the split kernels' fp32-accumulation error to a library conv's (tests/test_gpu_conv3x3.py), 1.1 the
bound of |SiLU'| (its maximum is 1.0998). There is no additive slack: the dropped al.bl term and the 2^-22 relative
split error are below E32.

tests/test_split_budget_cpu.py shows that the emulation keeps the budget and that every mutant breaks it;
tests/test_gpu_split_budget.py holds the kernels to it."""
from __future__ import annotations

import torch
import torch.nn.functional as F

# (B, Cin, Cout, H, W, k, stride): the smallest shapes that still cover each kernel's staging paths
CASES = [
    (2, 32, 32, 12, 20, 3, 1),    # stride-1 3x3: the 32-channel forms
    (1, 64, 64, 20, 20, 3, 1),
    (1, 256, 128, 9, 7, 3, 1),    # several chunks, ragged on both edges, W not a multiple of 4
    (2, 32, 64, 17, 39, 3, 2),    # stride-2 3x3: odd map
    (1, 96, 128, 8, 8, 3, 2),
    (3, 96, 256, 8, 8, 1, 1),     # 1x1: Cin below one stage, padded channels
    (1, 384, 256, 12, 12, 1, 1),  # three stages, tail tile
]
SCALES = (1.0, 2.0 ** -3, 2.0 ** -6, 1e-3)
WIDE_SCALES = (1.0, 2.0 ** -6)     # per-channel scales of 2^-10 .. 2^2 are used at these only
MUTANT_SCALES = (1.0, 2.0 ** -3, 2.0 ** -6)  # at 1e-3 the activations' low terms are at the floor themselves
MUTANTS = ("drop_xl", "drop_wl", "flush", "tap_wl", "chunk_xl")

X_FLOOR = 2.0 ** -25  # half the spacing of fp16's subnormals: an activation's low term
W_FLOOR = 2.0 ** -31  # the same for a weight, split as 64 W
WSC = 64.0            # csrc/split_conv.h SPLIT_WSC


def variants():
    """(s, wide) of every budget check of one case."""
    return [(s, False) for s in SCALES] + [(s, True) for s in WIDE_SCALES]


def make_case(B, Cin, Cout, H, W, k, stride, s, wide):
    """x [B, Cin, H, W] at scale s, w [Cout, Cin, k, k] at 1 / (k sqrt(Cin)), with ``wide`` per-channel scales of
    2^-10 .. 2^2 on both (as BN folding produces), and a bias that follows the signal (0.1 mean|x|)."""
    g = torch.Generator().manual_seed(B + Cin + Cout + H + W + k + stride)
    x = torch.randn(B, Cin, H, W, generator=g) * s
    w = torch.randn(Cout, Cin, k, k, generator=g) / (k * Cin ** 0.5)
    if wide:
        w = w * 2.0 ** (torch.rand(Cout, 1, 1, 1, generator=g) * 12 - 10)
        x = x * 2.0 ** (torch.rand(1, Cin, 1, 1, generator=g) * 12 - 10)
    b = torch.randn(Cout, generator=g) * 0.1 * x.abs().mean()
    return x.contiguous(), w.contiguous(), b


def gated(x, gate_c=None, gate_p=None):
    """(x * gate_c) * gate_p in fp32, the stride-2 kernel's documented order: gate_c [B, Cin], gate_p [B, H, W]."""
    y = x
    if gate_c is not None:
        y = y * gate_c[:, :, None, None]
    if gate_p is not None:
        y = y * gate_p[:, None]
    return y


def floor_sum(x_eff, w, k, stride):
    """The representation floor per output element, sum_k 2^-25 |w_nk| + 2^-31 |x_k|, in float64."""
    ax, aw = x_eff.double().abs(), w.double().abs()
    return (F.conv2d(torch.full_like(ax, X_FLOOR), aw, stride=stride, padding=k // 2)
            + F.conv2d(ax, torch.full_like(aw, W_FLOOR), stride=stride, padding=k // 2))


def budget(x, w, b, k, stride, gate_c=None, gate_p=None):
    """(ref64, lim): SiLU(conv(x_eff, w) + b) in float64 and the elementwise bound 8 E32 + 1.1 F of a split kernel's
    deviation from it."""
    assert x.dtype == torch.float32 and w.dtype == torch.float32 and not x.is_cuda
    x_eff = gated(x, gate_c, gate_p)
    ref64 = F.silu(F.conv2d(x_eff.double(), w.double(), b.double(), stride=stride, padding=k // 2))
    y32 = F.silu(F.conv2d(x_eff, w, b, stride=stride, padding=k // 2))
    e32 = float((y32.double() - ref64).abs().max())
    lim = 8.0 * e32 + 1.1 * floor_sum(x_eff, w, k, stride)
    return ref64, lim


def worst_ratio(y, ref64, lim):
    """max |y - ref64| / lim over the elements (the budget holds iff this is <= 1)."""
    return float(((y.double() - ref64).abs() / lim).max())


def _split(v):
    h = v.to(torch.float16).float()
    l = (v - h).to(torch.float16).float()  # v - h is exact in fp32
    return h, l


def emulate(x, w, b, k, stride, mutant=None):
    """The kernels' arithmetic on the CPU: fp16 h / l planes of x and of 64 w, the three products as fp32 convs summed
    smallest first, times 1/64, plus b, SiLU. ``mutant`` loses one term:
      drop_xl   no xl.wh product            drop_wl   no xh.wl product
      flush     low terms below 2^-14 (fp16 subnormals) are zero
      tap_wl    the weight low terms of tap (0, 0) are zero
      chunk_xl  the activation low terms of channels 0..31 are zero"""
    assert mutant is None or mutant in MUTANTS, mutant
    xh, xl = _split(x)
    wh, wl = _split(w * WSC)
    if mutant == "flush":
        xl = torch.where(xl.abs() < 2.0 ** -14, torch.zeros_like(xl), xl)
        wl = torch.where(wl.abs() < 2.0 ** -14, torch.zeros_like(wl), wl)
    elif mutant == "tap_wl":
        wl = wl.clone()
        wl[:, :, 0, 0] = 0
    elif mutant == "chunk_xl":
        xl = xl.clone()
        xl[:, :32] = 0
    conv = lambda a, c: F.conv2d(a, c, stride=stride, padding=k // 2)  # noqa: E731
    acc = torch.zeros(())
    if mutant != "drop_xl":
        acc = acc + conv(xl, wh)
    if mutant != "drop_wl":
        acc = acc + conv(xh, wl)
    acc = acc + conv(xh, wh)
    return F.silu(acc * (1.0 / WSC) + b[None, :, None, None])
