"""Test helper for the channel-attention ops (csrc/channel_attention.hip: SE, CBAM, CA) and the producers that feed
them plane statistics (csrc/conv_epilogue.hip, csrc/conv1x1x2_kernel.h). No GPU calls.

* ``part_plan``: the plane segmentation of the per-plane statistics, restated (yolosod_plane_parts).
* ``structured``: randn plus the structure random data lacks - entirely negative planes, pixel blocks negative in every
  channel, planes with an offset, outliers on both sides of every part boundary and on the last element.
* ``se_emul`` / ``cbam_emul`` / ``ca_emul``: the three ops in fp32 on the CPU in the kernels' summation order (plane
  partials per part, merged in k order; CBAM's 32-channel group sums, merged in g order; CA's four interleaved
  accumulators), with mutants that each lose one thing (``MUTANTS``).
* ``oracle`` / ``bound``: the fp64 oracle (oracle.model_ref.OP_CLASSES), the same module in fp32 on the CPU, and the
  bound   |y - ref64| <= K E32 + 2^-23 |ref64|   with E32 = max |ref32 - ref64|  (DESIGN.md section 29).

tests/test_channel_attn_cpu.py shows that the emulation keeps the bound on every case and that every mutant breaks
it on a case that can reach it; tests/test_gpu_channel_attn.py holds the kernels to it."""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

import recipes
from oracle.model_ref import OP_CLASSES
from yolosod_amd.nn import modules as M

# One K for all three ops: the next power of two above the worst ratio max|y - ref64| / E32 of the emulation (CPU) and of
# the kernels (MI355X), both listed in DESIGN.md section 29; 8 is the ceiling (the project's ratio for its own
# fp32-accumulation kernels against a library op, tests/split_budget.py).
K = 4.0

MUTANTS = ("max_init0", "pad_neg_inf", "drop_last_part", "mean_padded", "chan_tail", "group_tail", "ca_col_hi",
           "relu_swallows_nan")

# (shape, reduction, bf16 too): SE_Block(reduction), hid = max(C // r, 4)
SE_CASES = [
    ((2, 35, 9, 7), 5, False),        # hid = 7, channel tail 3, scalar HW
    ((2, 64, 12, 12), 1, True),       # hid = 64, the limit
    ((1, 264, 8, 8), 16, False),      # C > 256
    ((1, 8, 128, 128), 16, False),    # 2 parts
    ((1, 8, 130, 126), 16, False),    # 16380: 1 part
    ((1, 8, 131, 127), 16, False),    # odd HW, 2 parts: the scalar multi-part path
    ((1, 8, 172, 143), 16, True),     # 3 parts, seg rounded to 8200, short last part, vectors straddle rows
    ((1, 16, 256, 255), 16, False),   # fused apply
    ((1, 16, 256, 256), 16, False),   # split gate launch
]
SE_GATE_CASES = [SE_CASES[0], SE_CASES[3], SE_CASES[5]]
# CBAM_Block(C, None, ratio), hid = C // ratio
CBAM_CASES = [
    ((2, 35, 65, 17), 8, False),      # hid = 4, group of 3, G = 2, apply tail, odd HW, second sa tile in x and y
    ((2, 40, 68, 20), 8, True),       # hid = 5, group of 8 with the prefetch on
    ((2, 36, 20, 20), 36, False),     # hid = 1, group of 4 with the prefetch off
    ((1, 160, 12, 12), 16, False),    # G = 5
    ((1, 264, 8, 8), 8, False),       # G = 9, hid = 33, C > 256
    ((1, 128, 8, 8), 2, False),       # hid = 64
    ((1, 8, 131, 127), 2, False),     # multi-part scalar
    ((1, 8, 172, 143), 2, True),      # multi-part with a short last part
    ((1, 8, 1, 5), 2, False),         # degenerate
]
CBAM_GATE_CASES = [CBAM_CASES[0], CBAM_CASES[6]]
# CA_Block(C, None, reduction), mip = max(8, C // reduction)
CA_CASES = [
    ((2, 36, 9, 7), 4, False),        # mip = 9, C % 4 == 0 but the mip tail, L = 16
    ((2, 35, 13, 10), 32, False),     # C % 4 = 3, L = 23
    ((1, 136, 8, 12), 32, True),      # second staging iteration
    ((1, 8, 20, 1024), 32, True),     # RB = 8, ragged last band, col[3], V = 4 and the bf16 V = 8
    ((1, 8, 3, 1021), 32, False),     # odd W > 768
    ((1, 8, 5, 300), 32, False),      # col[1]
]
CASES = {"SE_Block": SE_CASES, "CBAM_Block": CBAM_CASES, "CA_Block": CA_CASES}
# Offset and outliers of ``structured``. At +100 / +-50 the gates saturate under the recipe parameters (live, i.e. in
# (0.001, 0.999): 6-27 % of the SE gates, 0-15 % of CBAM's ca, 0-35 % of CA's hidden activations inside the clamp), so
# most gate arithmetic went unchecked: the max_init0 mutant passed at CBAM 2x35x65x17 (ratio 0.19), and at SE 1x8x130x126
# one live gate was left, whose error is a single rounding of the +100 plane's mean (half an ulp of 100 = 3.8e-6): E32
# came out at 3.6e-7 and an emulation with the better mean at 41 E32. At 1/8 of that 38-100 % / 14-100 % / 12-73 % are
# live, every mutant is shown, and E32 is the product rounding of the largest outputs on every case.
OFFSET, OUTLIER = 12.5, 6.25
NAN_SHAPES = [(2, 35, 9, 7), (2, 40, 12, 12)]  # one scalar, one vector; the NaN goes to x[NAN_AT]
NAN_AT = (1, 3, 2, 4)
NAN_ARG = {"SE_Block": 5, "CBAM_Block": 8, "CA_Block": 4}


def case_id(c):
    return "x".join(map(str, c[0])) + f"-r{c[1]}"


def part_plan(HW: int):
    """(parts, seg) of channel_attention.hip's part_plan."""
    p = min(max(HW // 8192, 1), 64)
    seg = (HW + p - 1) // p
    if HW % 4 == 0:
        seg = (seg + 3) & ~3
    return (HW + seg - 1) // seg, seg


# With the plain seed the single hidden unit of the hid = 1 case is dead in both branches (W1 avg = -5.1, W1 max = -14.1):
# ca = 0.5 in every channel and the chan_tail mutant passed. With this salt W1 avg = 0.5 (alive) and W1 max = -15 (cut).
SALT = {("CBAM_Block", 36, 36): "d"}


def seed_of(op, C, arg):
    """Seed of the recipe parameters of ``op`` with C channels and constructor argument ``arg``."""
    return recipes.seed_of(f"{SALT.get((op, C, arg), '')}{op}-{C}-{arg}")


def input_seed(op, shape, arg):
    return seed_of(op, shape[1], arg) + 1 + 1000 * shape[2] + shape[3]


def structured(shape, seed):
    """randn [B, C, H, W] plus: (c) every fifth plane + OFFSET; (a) every third plane entirely negative; (d) +-OUTLIER
    at flat indices HW - 1, k seg - 1 and k seg of every part boundary (-OUTLIER in the negative planes, so they stay
    negative); (b) a 5x5 block at the top-left corner and an interior one negative in all channels."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    neg = -torch.randn(shape, generator=g).abs() - 0.5
    x[:, 0::5] += OFFSET
    x[:, 2::3] = neg[:, 2::3]
    parts, seg = part_plan(H * W)
    xf = x.view(B, C, H * W)
    sgn = torch.ones(C)
    sgn[2::3] = -1.0
    for j, i in enumerate([H * W - 1] + [k * seg - d for k in range(1, parts) for d in (1, 0)]):
        xf[:, :, i] = OUTLIER * torch.where(sgn < 0, sgn, sgn * (1.0 if j % 2 == 0 else -1.0))
    r0, c0 = min(max(H // 4, 1), max(H - 5, 0)), min(W // 2, max(W - 5, 0))
    for r, c in ((0, 0), (r0, c0)):
        x[:, :, r:r + 5, c:c + 5] = neg[:, :, r:r + 5, c:c + 5]
    return x.contiguous()


def with_nan(x):
    x = x.clone()
    x[NAN_AT] = float("nan")
    return x


# ---- modules and the oracle -------------------------------------------------------------------------------------

def build(op, arg, C, classes=None, seed=None):
    """The product module (or, with classes=OP_CLASSES, the oracle's) with recipe parameters, on the CPU in fp32."""
    cls = (classes or {}).get(op) or getattr(M, op)
    m = cls(arg) if op == "SE_Block" else cls(C, None, arg)
    if op == "SE_Block":
        m._maybe_build(C, None)
    recipes.perturb_(m, seed_of(op, C, arg) if seed is None else seed)
    return m.eval()


@functools.lru_cache(maxsize=None)
def case_data(op, shape, arg):
    """(x, ref64, E32) of a case: the structured input, the fp64 oracle and the fp32 oracle's error. Computed once and
    shared; callers must not modify them."""
    x = structured(shape, input_seed(op, shape, arg))
    return (x,) + oracle(op, arg, x)


def oracle(op, arg, x):
    m = build(op, arg, x.shape[1], OP_CLASSES)
    with torch.inference_mode():
        ref32 = m(x).double()
        ref64 = m.double()(x.double())
    return ref64, float((ref32 - ref64).abs().max())


def oracle_bf16(op, arg, x):
    """The fp64 oracle on bf16-rounded parameters and input (tests/test_gpu_bf16.py's reference)."""
    m = build(op, arg, x.shape[1], OP_CLASSES).to(torch.bfloat16).double()
    with torch.inference_mode():
        return m(x.to(torch.bfloat16).double())


def oracle_gates(op, arg, x):
    """The gates of the oracle in fp64 and their fp32 error: SE -> [(a [B, C], E32)], CBAM -> [(ca, E32), (sa, E32)]."""
    m = build(op, arg, x.shape[1], OP_CLASSES)

    def run(m, x):
        if op == "SE_Block":
            a = F.relu(F.conv2d(F.adaptive_avg_pool2d(x, 1), m.fc1.weight, m.fc1.bias))
            return [torch.sigmoid(F.conv2d(a, m.fc2.weight, m.fc2.bias)).flatten(1)]
        fc = m.channel_attention.fc
        ca = torch.sigmoid(fc(F.adaptive_avg_pool2d(x, 1)) + fc(F.adaptive_max_pool2d(x, 1)))
        o = ca * x
        s = torch.cat([o.mean(1, keepdim=True), o.max(1, keepdim=True)[0]], 1)
        sa = torch.sigmoid(F.conv2d(s, m.spatial_attention.conv1.weight, padding=3))
        return [ca.flatten(1), sa[:, 0]]

    with torch.inference_mode():
        g32 = [t.double() for t in run(m, x)]
        g64 = run(m.double(), x.double())
    return [(b, float((a - b).abs().max())) for a, b in zip(g32, g64)]


def bound(ref64, e32, k=K):
    return k * e32 + 2.0 ** -23 * ref64.abs()


def worst_ratio(y, ref64, e32, k=K):
    """max |y - ref64| / bound; inf when y is not finite where the reference is (or differs in NaN mask)."""
    y = y.double()
    if not torch.equal(torch.isnan(y), torch.isnan(ref64)):
        return float("inf")
    ok = ~torch.isnan(ref64)
    if not bool(ok.any()):
        return 0.0
    r = ((y - ref64).abs() / bound(ref64, e32, k))[ok].max()
    return float("inf") if torch.isnan(r) else float(r)


def e32_ratio(y, ref64, e32):
    """max |y - ref64| / E32: the figure K is chosen from."""
    return float((y.double() - ref64).abs().max()) / e32


# ---- fp32 emulation in the kernels' order ---------------------------------------------------------------------------

def _nmax(a, b, swallow):
    return torch.fmax(a, b) if swallow else torch.maximum(a, b)


def _amax(t, dim, swallow):
    return t.nan_to_num(nan=float("-inf")).amax(dim) if swallow else t.amax(dim)


def _relu(t, swallow):
    return _nmax(t, torch.zeros((), dtype=t.dtype), swallow)


def plane_stats(x, mutant=None):
    """(avg, max) [B, C] of the planes: one partial per part, merged in k order (plane_part_stats_kernel, gate_mlp)."""
    B, C, H, W = x.shape
    HW = H * W
    parts, seg = part_plan(HW)
    sw = mutant == "relu_swallows_nan"
    xf = x.reshape(B, C, HW)
    s = torch.zeros(B, C)
    m = torch.full((B, C), 0.0 if mutant == "max_init0" else float("-inf"))
    for k in range(parts - 1 if mutant == "drop_last_part" and parts > 1 else parts):
        part = xf[:, :, k * seg:min((k + 1) * seg, HW)]
        s = s + part.sum(-1)
        m = _nmax(m, _amax(part, -1, sw), sw)
    inv = torch.tensor(1.0) / torch.tensor(float(parts * seg if mutant == "mean_padded" else HW))
    return s * inv, m


def _chan_tail(gate, mutant):
    C = gate.shape[1]
    if mutant == "chan_tail" and C % 8:
        gate = gate.clone()
        gate[:, C // 8 * 8:] = gate[:, :1]
    return gate


def se_emul(m, x, mutant=None):
    """(y, gate) of SE in fp32."""
    sw = mutant == "relu_swallows_nan"
    w1, w2 = m.fc1.weight.flatten(1), m.fc2.weight.flatten(1)
    avg, _ = plane_stats(x, mutant)
    h = _relu(avg @ w1.t() + m.fc1.bias, sw)
    gate = torch.sigmoid(h @ w2.t() + m.fc2.bias)
    return x * _chan_tail(gate, mutant)[:, :, None, None], gate


def cbam_emul(m, x, mutant=None):
    """(y, ca, sa) of CBAM in fp32: pixel statistics per 32-channel group in channel order, groups merged in g order."""
    sw = mutant == "relu_swallows_nan"
    B, C, H, W = x.shape
    fc = m.channel_attention.fc
    w1, w2 = fc[0].weight.flatten(1), fc[2].weight.flatten(1)
    avg, mx = plane_stats(x, mutant)
    ca = torch.sigmoid(_relu(avg @ w1.t(), sw) @ w2.t() + _relu(mx @ w1.t(), sw) @ w2.t())
    o = ca[:, :, None, None] * x
    init = 0.0 if mutant == "max_init0" else float("-inf")
    s, mm = torch.zeros(B, H, W), torch.full((B, H, W), init)
    for c0 in range(0, C, 32):
        c1 = min(c0 + 32, C)
        if mutant == "group_tail" and c1 - c0 < 32 and c0 > 0:
            continue
        sg, mg = torch.zeros(B, H, W), torch.full((B, H, W), init)
        for c in range(c0, c1):
            sg = sg + o[:, c]
            mg = _nmax(mg, o[:, c], sw)
        s = s + sg
        mm = _nmax(mm, mg, sw)
    mean = s * (torch.tensor(1.0) / torch.tensor(float(C)))
    pad = F.pad(torch.stack([mean, mm], 1), (3, 3, 3, 3))
    if mutant == "pad_neg_inf":
        inside = F.pad(torch.ones(B, 1, H, W, dtype=torch.bool), (3, 3, 3, 3))
        pad[:, 1:2] = torch.where(inside, pad[:, 1:2], torch.tensor(float("-inf")))
    sa = torch.sigmoid(F.conv2d(pad, m.spatial_attention.conv1.weight))[:, 0]
    y = sa[:, None] * (_chan_tail(ca, mutant)[:, :, None, None] * x)
    return y, ca, sa


def _fma(a, b, c):
    """fmaf in fp32: the product of two fp32 values is exact in fp64."""
    return (a.double() * b.double() + c.double()).float()


def ca_emul(m, x, mutant=None):
    """y of CA in fp32: row means by lane quads, column sums row by row, conv1 with four interleaved fma accumulators
    over the channels (ca_pool_kernel, ca_gate_kernel)."""
    sw = mutant == "relu_swallows_nan"
    B, C, H, W = x.shape
    xp = F.pad(x, (0, (-W) % 4)).view(B, C, H, -1, 4)
    q = torch.zeros(B, C, H, 4)
    for i in range(xp.shape[3]):
        q = q + xp[:, :, :, i]
    rows = ((q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])) * (torch.tensor(1.0) / torch.tensor(float(W)))
    cols = torch.zeros(B, C, W)
    for h in range(H):
        cols = cols + x[:, :, h]
    cols = cols * (torch.tensor(1.0) / torch.tensor(float(H)))
    if mutant == "ca_col_hi":
        cols[:, :, 256:] = 0.0
    yin = torch.cat([rows, cols], 2)                       # [B, C, L]
    w1 = m.conv1.weight.flatten(1)                         # [mip, C]
    acc = [torch.zeros(B, w1.shape[0], H + W) for _ in range(4)]
    for c in range(C):
        u = c % 4 if c < C // 4 * 4 else 0
        acc[u] = _fma(w1[None, :, c, None], yin[:, None, c], acc[u])
    z = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + m.conv1.bias[None, :, None]
    bn = m.bn1
    inv = 1.0 / torch.sqrt(bn.running_var + bn.eps)
    z = (z - bn.running_mean[None, :, None]) * inv[None, :, None] * bn.weight[None, :, None] + bn.bias[None, :, None]
    z = z + 3.0
    if sw:
        t = torch.fmin(torch.fmax(z, torch.tensor(0.0)), torch.tensor(6.0)) / 6.0
    else:
        t = torch.minimum(torch.maximum(z, torch.tensor(0.0)), torch.tensor(6.0)) / 6.0
    wh, ww = m.conv_h.weight.flatten(1), m.conv_w.weight.flatten(1)      # [C, mip]
    ah, aw = torch.zeros(B, C, H), torch.zeros(B, C, W)
    for j in range(w1.shape[0]):
        ah = ah + wh[None, :, j, None] * t[:, None, j, :H]
        aw = aw + ww[None, :, j, None] * t[:, None, j, H:]
    ah = torch.sigmoid(ah + m.conv_h.bias[None, :, None])
    aw = torch.sigmoid(aw + m.conv_w.bias[None, :, None])
    return (x * aw[:, :, None, :]) * ah[:, :, :, None]


def emulate(op, arg, x, mutant=None):
    """y of ``op`` in fp32 in the kernels' order (recipe parameters)."""
    m = build(op, arg, x.shape[1])
    with torch.inference_mode():
        if op == "SE_Block":
            return se_emul(m, x, mutant)[0]
        if op == "CBAM_Block":
            return cbam_emul(m, x, mutant)[0]
        return ca_emul(m, x, mutant)
