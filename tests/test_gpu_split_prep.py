"""The prepared weight block of the fp16-split conv kernels (csrc/split_conv.h): one format, written by
split_prep_kernel and read by conv3x3.hip (the fused Bottleneck included), conv3x3s2.hip and conv1x1x2.hip.

The block is two 256-byte-rounded regions: the 2 Cout cin_pad taps fp16 values and one flag word. Element (n, k, t) of
W [Cout][Cin][taps] (cin_pad = Cin for the 3x3 convs, Cin rounded up to 128 with zero channels for the 1x1 conv) has
the high term of 64 W at half
    ((t nq + q) ncb + cb) 1024 + ln 8 + (kk & 7),   q = k >> 5, kk = k & 31, cb = n >> 4, ln = ((kk >> 3) << 4) + (n & 15),
with nq = cin_pad / 32 and ncb = Cout / 16, and the low term 512 halves further.

The weights are small integers over 64: 64 W is exact in fp16, so the high plane holds the integer, the low plane 0,
and the comparison is bit for bit. Shapes: the smallest that exercise every index field."""
import numpy as np
import pytest
import torch

from yolosod_amd import _hip

# name: (prepare, size query, Cout, Cin, taps, cin_pad)
CASES = {
    "conv3x3": ("conv3x3_prepare", "yolosod_conv3x3_prep_bytes_ex", 32, 64, 9, 64),
    "conv3x3s2": ("conv3x3s2_prepare", "yolosod_conv3x3s2_prep_bytes", 64, 32, 9, 32),
    "conv1x1x2_pad": ("conv1x1x2_prepare", "yolosod_conv1x1x2_prep_bytes", 64, 96, 1, 128),
    "conv1x1x2": ("conv1x1x2_prepare", "yolosod_conv1x1x2_prep_bytes", 128, 128, 1, 128),
}
UNSUPPORTED = {"yolosod_conv3x3_prep_bytes_ex": (48, 64), "yolosod_conv3x3s2_prep_bytes": (32, 96),
               "yolosod_conv1x1x2_prep_bytes": (96, 192)}  # (Cin, Cout)


def _round256(nbytes):
    return (nbytes + 255) // 256 * 256


def _weights(cout, cin, taps):
    n, k, t = np.meshgrid(np.arange(cout), np.arange(cin), np.arange(taps), indexing="ij")
    return ((((n * cin + k) * taps + t) % 2039 - 1019) / 64).astype(np.float32)


def _expected(w, cin_pad):
    cout, cin, taps = w.shape
    nq, ncb = cin_pad // 32, cout // 16
    n, k, t = np.meshgrid(np.arange(cout), np.arange(cin), np.arange(taps), indexing="ij")
    q, kk, cb = k >> 5, k & 31, n >> 4
    ln = ((kk >> 3) << 4) + (n & 15)
    base = ((t * nq + q) * ncb + cb) * 1024 + ln * 8 + (kk & 7)
    exp = np.zeros(2 * cout * cin_pad * taps, dtype=np.float16)  # low plane and padded channels: + 0
    exp[base.ravel()] = (64 * w).astype(np.float16).ravel()
    assert np.array_equal(exp[base.ravel()].astype(np.float32), 64 * w.ravel())  # 64 W is exact in fp16
    return exp


@pytest.mark.parametrize("name", list(CASES))
def test_prep_bytes_is_two_rounded_regions(name):
    _, query, cout, cin, taps, cin_pad = CASES[name]
    lib = _hip.load_library()
    assert getattr(lib, query)(cin, cout) == _round256(2 * cout * cin_pad * taps * 2) + 256
    assert getattr(lib, query)(*UNSUPPORTED[query]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_prepared_block_layout(name, cuda):
    prepare, _, cout, cin, taps, cin_pad = CASES[name]
    w = _weights(cout, cin, taps)
    wt = torch.from_numpy(w).to(cuda)
    blk = getattr(_hip, prepare)(wt.reshape(cout, cin, 3, 3) if taps == 9 else wt.reshape(cout, cin, 1, 1))
    torch.cuda.synchronize()
    halves = 2 * cout * cin_pad * taps
    assert blk.dtype == torch.uint8 and blk.numel() == _round256(2 * halves) + 256
    raw = blk.cpu().numpy()
    got = raw[:2 * halves].view(np.uint16)
    exp = _expected(w, cin_pad).view(np.uint16)
    assert np.array_equal(got, exp), f"{int((got != exp).sum())} of {halves} halves differ"
    assert raw[_round256(2 * halves):][:4].view(np.uint32)[0] == 0  # the block's range word: 64 W within fp16's range
