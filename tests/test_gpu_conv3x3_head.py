"""GPU: a Detect tower's last 3x3 conv with the tower's 1x1 conv and the decode in its epilogue (csrc/conv3x3.hip,
conv3x3_head_kernel) against the two steps it replaces, the stride-1 fp16-split conv followed by the head kernel on that
level: bit-identical in both modes on every tile geometry, on ragged maps, with a workgroup walking several tiles, for
nc 1 / 10 / 16 and the level at the first, a middle and the last anchor offset; every element of y the launch does not
own stays NaN; the input may be a channel slice between NaN channels; the split-range flag; the fp64 bound of
tests/test_gpu_ops.py::test_detect_head_fused_vs_oracle."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oplib import tol_close
from oracle import ops_ref as R
from yolosod_amd import _hip

pytestmark = pytest.mark.gpu

MAPS = [(2, 8, 32),     # one exact 32 x 8 tile
        (2, 12, 20),    # the 20 x 12 tile of 4 x 4 blocks
        (2, 6, 40),     # the 40 x 6 tile of 8 x 2 blocks
        (2, 24, 44),    # ragged in both directions
        (2, 40, 36),
        (1, 4, 4)]      # smaller than a tile
BIG = (6, 160, 160)     # 600 tiles on 512 workgroup slots: a workgroup walks several tiles
STRIDES = [4.0, 8.0, 16.0, 32.0]
OTHER = [(4, 8), (2, 4), (4, 4)]  # the map sizes of the three levels around the one under test


class forced_form:
    """yolosod_debug_set_conv3x3_form: geometry 1 .. 3 (0: automatic); the head launch always runs 64-channel groups."""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        self.old = _hip.load_library().yolosod_debug_set_conv3x3_form(self.form)

    def __exit__(self, *exc):
        _hip.load_library().yolosod_debug_set_conv3x3_form(self.old)


def _layout(H, W, li):
    hw = list(OTHER)
    hw.insert(li, (H, W))
    offs = [0]
    for h, w in hw:
        offs.append(offs[-1] + h * w)
    return hw, offs


@functools.lru_cache(maxsize=None)
def _case(shape, nc=10, li=1):
    """One level under test at index li of a four-level layout: operands, prepared blocks, and the reference y (NaN
    outside the level) from conv3x3_silu + detect_head_into of that level. Computed once, never modified."""
    B, H, W = shape
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(B * 10007 + H * 101 + W + nc * 7 + li)
    hw, offs = _layout(H, W, li)
    # the input: channels 64 .. 127 of a 192-channel buffer, NaN around them and in a neighbouring image
    z = torch.full((B + 1, 192, H, W), float("nan"))
    z[:B, 64:128] = torch.randn(B, 64, H, W, generator=g)
    z = z.to(dev)
    x = z[:B, 64:128]
    c = dict(shape=shape, nc=nc, li=li, hw=hw, offs=offs, A=offs[-1], z=z, x=x, stride=STRIDES[li])
    for m in (1, 2):  # box / class tower
        rows = 64 if m == 1 else nc
        c[f"w{m}"] = (torch.randn(64, 64, 3, 3, generator=g) / (3 * 8.0)).to(dev)
        c[f"b{m}"] = (torch.randn(64, generator=g) * 0.5).to(dev)
        c[f"hw{m}"] = (torch.randn(rows, 64, generator=g) * (0.25 if m == 1 else 0.2)).to(dev)
        c[f"hb{m}"] = (torch.randn(rows, generator=g) - (0.0 if m == 1 else 2.0)).to(dev)
        c[f"p{m}"] = _hip.conv3x3_prepare(c[f"w{m}"])
        c[f"hp{m}"] = _hip.detect_head_prepare(c[f"hw{m}"], rows)
    c["ref"] = _reference(c)
    return c


def _reference(c, x=None, b1=None, hw1=None):
    """The two steps: both towers' conv launches, then the head kernel on the level alone (the registered op, the other
    levels' features dummies that it does not read)."""
    B = c["shape"][0]
    x = c["x"] if x is None else x
    fb = _hip.conv3x3_silu(x, c["b1"] if b1 is None else b1, lambda: c["p1"], 64)
    fc = _hip.conv3x3_silu(x, c["b2"], lambda: c["p2"], 64)
    fbs, fcs, wb, bb, wc, bc = [], [], [], [], [], []
    for i, (h, w) in enumerate(c["hw"]):
        own = i == c["li"]
        fbs.append(fb if own else torch.zeros(B, 64, h, w, device=x.device))
        fcs.append(fc if own else torch.zeros(B, 64, h, w, device=x.device))
        wb.append(c["hw1"] if hw1 is None else hw1)
        bb.append(c["hb1"])
        wc.append(c["hw2"])
        bc.append(c["hb2"])
    y = torch.full((B, 4 + c["nc"], c["A"]), float("nan"), device=x.device)
    _hip.detect_head_into(y, c["li"], c["li"] + 1, fbs, fcs, wb, bb, wc, bc, STRIDES, c["nc"])
    return y


def _fused(c, y, mode, x=None, b1=None, hp1=None, hw1=None):
    x = c["x"] if x is None else x
    bias = c[f"b{mode}"] if (mode == 2 or b1 is None) else b1
    hp = c[f"hp{mode}"] if (mode == 2 or hp1 is None) else hp1
    return _hip.conv3x3_head(x, bias, lambda: c[f"p{mode}"], lambda: hp, c[f"hb{mode}"], mode, c["nc"], c["stride"], y,
                             c["offs"][c["li"]])


def _same(a, b):
    """Bit equality where NaN equals NaN."""
    return torch.equal(torch.nan_to_num(a, nan=-12345.0), torch.nan_to_num(b, nan=-12345.0)) and torch.equal(
        torch.isnan(a), torch.isnan(b))


def _check(c):
    B, nc, A = c["shape"][0], c["nc"], c["A"]
    a0, a1 = c["offs"][c["li"]], c["offs"][c["li"] + 1]
    ref = c["ref"]
    assert torch.isfinite(ref[:, :, a0:a1]).all() and torch.isnan(ref[:, :, :a0]).all() and torch.isnan(
        ref[:, :, a1:]).all()
    _hip.split_range_flag(reset=True)
    y = torch.full((B, 4 + nc, A), float("nan"), device=ref.device)
    _fused(c, y, 1)
    own = torch.zeros_like(y, dtype=torch.bool)
    own[:, :4, a0:a1] = True
    assert torch.isnan(y[~own]).all(), "box mode wrote outside its rows / anchors"
    d = (y[:, :4, a0:a1] - ref[:, :4, a0:a1]).abs().max()
    assert torch.equal(y[:, :4, a0:a1], ref[:, :4, a0:a1]), f"box: max |d| {float(d):.3g}"
    _fused(c, y, 2)
    own[:, 4:, a0:a1] = True
    assert torch.isnan(y[~own]).all(), "class mode wrote outside its rows / anchors"
    d = (y[:, 4:, a0:a1] - ref[:, 4:, a0:a1]).abs().max()
    assert torch.equal(y[:, 4:, a0:a1], ref[:, 4:, a0:a1]), f"class: max |d| {float(d):.3g}"
    assert _same(y, ref)
    assert not _hip.split_range_flag(reset=True)
    # the input's surroundings are untouched
    z, xb = c["z"], c["shape"][0]
    assert torch.isnan(z[:xb, :64]).all() and torch.isnan(z[:xb, 128:]).all() and torch.isnan(z[xb]).all()


@pytest.mark.parametrize("geo", [1, 2, 3])
@pytest.mark.parametrize("shape", MAPS)
def test_equals_conv_then_head(shape, geo, cuda):
    c = _case(shape)
    with forced_form(geo):
        _check(c)


def test_a_workgroup_walks_several_tiles(cuda):
    _check(_case(BIG))


@pytest.mark.parametrize("nc", [1, 16])
def test_class_counts(nc, cuda):
    _check(_case((2, 24, 44), nc=nc))


@pytest.mark.parametrize("li", [0, 3])
def test_first_and_last_anchor_offset(li, cuda):
    _check(_case((2, 24, 44), li=li))


def test_prepared_head_planes_are_the_head_kernels(cuda):
    """The prepared block is the hi plane then the lo plane of split2(64 W) in [t][s][g][row][i] order, class rows past
    nc zero (what detect_head_x2_kernel builds per workgroup), and its range word is clear."""
    c = _case((2, 24, 44))
    for m, rows, nt in ((1, 64, 4), (2, c["nc"], 1)):
        w = c[f"hw{m}"].cpu()
        wp = torch.zeros(16 * nt, 64)
        wp[:rows] = w
        v = (wp * 64.0).view(nt, 16, 2, 8, 4).permute(0, 2, 4, 1, 3).contiguous()  # [t][row][s][i][g] -> [t][s][g][row][i]
        hi = v.half()
        lo = (v - hi.float()).half()
        blk = c[f"hp{m}"].cpu()
        n = nt * 1024
        got = blk[:4 * n].view(torch.float16)
        assert torch.equal(got[:n].view(torch.int16), hi.reshape(-1).view(torch.int16)), m
        assert torch.equal(got[n:].view(torch.int16), lo.reshape(-1).view(torch.int16)), m
        assert int(blk[-256:-252].view(torch.int32)) == 0


def test_split_range_flag(cuda):
    c = _case((2, 24, 44))
    B, nc, A = 2, c["nc"], c["A"]
    y = torch.full((B, 4 + nc, A), float("nan"), device=cuda)
    _hip.split_range_flag(reset=True)
    for mode in (1, 2):
        _fused(c, y, mode)
        assert not _hip.split_range_flag(reset=True)
    # the staged input leaves fp16's range
    xb = c["x"].clone()
    xb[1, 7, 13, 21] = 1e6
    for mode in (1, 2):
        _fused(c, y, mode, x=xb)
        assert _hip.split_range_flag(reset=True), mode
    # a feature above fp16's range: SiLU(conv + 1e5) ~ 1e5; the conv launch alone does not flag, the head does
    big_b = c["b1"].clone()
    big_b[3] = 1e5
    f = _hip.conv3x3_silu(c["x"], big_b, lambda: c["p1"], 64)
    assert not _hip.split_range_flag(reset=True) and float(f.max()) > 65504.0
    _reference(c, b1=big_b)
    assert _hip.split_range_flag(reset=True)
    _fused(c, y, 1, b1=big_b)
    assert _hip.split_range_flag(reset=True)
    # a head weight above range: the prepared block's own flag is re-reported by every launch
    hw_big = c["hw1"].clone()
    hw_big[5, 9] = 2000.0
    hp_big = _hip.detect_head_prepare(hw_big, 64)
    assert _hip.split_range_flag(reset=True)  # the preparation itself reports
    _fused(c, y, 1, hp1=hp_big)
    assert _hip.split_range_flag(reset=True)
    _fused(c, y, 1)
    assert not _hip.split_range_flag(reset=True)


def test_matches_fp64(cuda):
    """The bound of tests/test_gpu_ops.py::test_detect_head_fused_vs_oracle (5e-4 absolute + 1e-5 relative) against a
    double-precision reference of the whole chain: conv3x3 + SiLU, the 1x1 convs, decode_ref."""
    c = _case((2, 24, 44))
    B, nc = 2, c["nc"]
    xd = c["x"].cpu().double()
    maps = []
    for i, (h, w) in enumerate(c["hw"]):
        if i != c["li"]:
            maps.append(torch.zeros(B, 64 + nc, h, w, dtype=torch.float64))
            continue
        parts = []
        for m in (1, 2):
            f = F.silu(F.conv2d(xd, c[f"w{m}"].cpu().double(), c[f"b{m}"].cpu().double(), padding=1))
            parts.append(torch.einsum("ok,bkhw->bohw", c[f"hw{m}"].cpu().double(), f)
                         + c[f"hb{m}"].cpu().double().view(1, -1, 1, 1))
        maps.append(torch.cat(parts, 1))
    ref = R.decode_ref(maps, STRIDES, nc)
    a0, a1 = c["offs"][c["li"]], c["offs"][c["li"] + 1]
    y = torch.full((B, 4 + nc, c["A"]), float("nan"), device=cuda)
    _fused(c, y, 1)
    _fused(c, y, 2)
    ok, err, ratio = tol_close(y[:, :, a0:a1].cpu(), ref[:, :, a0:a1], 5e-4, 1e-5)
    print(f"fused conv + head vs fp64: max abs err {err:.3g}, worst ratio to the bound {ratio:.3f}")
    assert ok, f"max abs err {err:.3g} (ratio {ratio:.3f})"


def test_head_into_with_sizes_for_absent_levels(cuda):
    """detect_head_into with map sizes in place of the features of levels outside the range (the executor's call when
    those levels were decoded by their towers) equals the call with tensors."""
    c = _case((2, 24, 44))
    B, nc = 2, c["nc"]
    fb = _hip.conv3x3_silu(c["x"], c["b1"], lambda: c["p1"], 64)
    fc = _hip.conv3x3_silu(c["x"], c["b2"], lambda: c["p2"], 64)
    fbs = [fb if i == c["li"] else hw for i, hw in enumerate(c["hw"])]
    fcs = [fc if i == c["li"] else None for i in range(4)]
    y = torch.full((B, 4 + nc, c["A"]), float("nan"), device=cuda)
    with _hip.op_timer() as t:
        _hip.detect_head_into(y, c["li"], c["li"] + 1, fbs, fcs, [c["hw1"]] * 4, [c["hb1"]] * 4, [c["hw2"]] * 4,
                              [c["hb2"]] * 4, STRIDES, nc)
    assert _same(y, c["ref"])
    (key, _), = t.durations_ms()
    assert key == ("head", (B, 24 * 44), (nc, 64, 64))  # the anchors it decodes, not the layout's


def test_bad_arguments_are_errors(cuda):
    c = _case((2, 24, 44))
    y = torch.full((2, 4 + c["nc"], c["A"]), float("nan"), device=cuda)
    with pytest.raises(RuntimeError):
        _hip.conv3x3_head(c["x"][:, :, :, :42], c["b1"], lambda: c["p1"], lambda: c["hp1"], c["hb1"], 1, c["nc"], 8.0,
                          y, 0)  # W % 4 != 0 (and not an image view)
    with pytest.raises(RuntimeError):
        _fused(c, y[:, :, :100].contiguous(), 1)  # the level's anchors do not fit
    with pytest.raises(RuntimeError):
        _hip.conv3x3_head(c["x"], c["b1"], lambda: c["p1"], lambda: c["hp1"], c["hb1"], 3, c["nc"], 8.0, y, 0)
    assert torch.isnan(y).all()
