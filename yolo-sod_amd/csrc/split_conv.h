// What the fp16-split conv kernels (conv3x3.hip, conv3x3s2.hip, conv1x1x2.hip) share: the prepared weight block (its
// layout, the kernel that writes it and the host path that runs that kernel) and the launch arithmetic of the
// persistent grids. The block is a format that every one of those kernels reads, so it is defined here once.
//
// Prepared block of W [Cout][Cin][TAPS] (TAPS 9: a 3x3 conv, 1: a 1x1 conv whose Cin is padded with zero channels to
// cin_pad): two 256-byte-rounded regions, 2 Cout cin_pad TAPS fp16 values and one flag word. The values are the
// two-term split of 64 W in fragment-major planes: for tap t, 32-channel input chunk q (of nq = cin_pad / 32),
// 16-channel output block cb (of ncb = Cout / 16) and plane p (0: high terms, 1: low terms), the 64 lanes' MFMA
// fragments (lane (g, l15): output channel 16 cb + l15, input channels 32 q + 8 g .. + 7) are 1 KB contiguous at
// half (((t nq + q) ncb + cb) 2 + p) 512. The flag word records whether 64 W left fp16's range; every conv launch
// re-reports it into the device's split-range flag.
#pragma once
#include "common.h"

namespace ys {

constexpr float SPLIT_WSC = 64.0f;  // weight scale (exact, a power of two): the low terms stay normal fp16

struct SplitPrep {
  h16_t* wp;       // the planes
  unsigned* flag;  // the block's own range word
};
inline size_t split_prep_bytes(size_t halves) {
  Sizer s;
  s.take<h16_t>(halves);
  s.take<unsigned>(1);
  return s.off;
}
inline bool split_prep_carve(const void* buf, size_t bytes, size_t halves, SplitPrep* out) {
  Carver cv(const_cast<void*>(buf), bytes);
  out->wp = cv.take<h16_t>(halves);
  out->flag = cv.take<unsigned>(1);
  return out->flag != nullptr;
}

// One thread per (output channel n, padded input channel k, tap t).
template <int TAPS>
__global__ __launch_bounds__(256) void split_prep_kernel(const float* __restrict__ w, int cin, int cin_pad, int cout,
                                                         h16_t* __restrict__ wp, unsigned* range_flag,
                                                         unsigned* prep_flag) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)cout * cin_pad * TAPS) return;
  const int t = (int)(i % TAPS), k = (int)((i / TAPS) % cin_pad), n = (int)(i / ((long)TAPS * cin_pad));
  const float v = k < cin ? w[((long)n * cin + k) * TAPS + t] * SPLIT_WSC : 0.f;  // zero weights for padded channels
  const _Float16 hh = (_Float16)v;
  const _Float16 ll = (_Float16)(v - (float)hh);
  const int nq = cin_pad >> 5, q = k >> 5, kk = k & 31, cb = n >> 4, ncb = cout >> 4;
  const int ln = ((kk >> 3) << 4) + (n & 15);
  const long base = ((long)((t * nq + q) * ncb + cb) * 2) * 512 + ln * 8 + (kk & 7);
  wp[base] = __builtin_bit_cast(h16_t, hh);
  wp[base + 512] = __builtin_bit_cast(h16_t, ll);
  const float m = fabsf(v);
  range_report(range_flag, m);
  range_report(prep_flag, m);
}

// Weight preparation (re-run whenever the weights change): w [cout][cin][TAPS] fp32 (BN folded) -> prep block. The
// caller has checked the shape; `what` prefixes the error texts.
template <int TAPS>
int split_prepare(const char* what, const float* w, int cin, int cin_pad, int cout, void* prep, size_t prep_bytes,
                  void* stream) {
  YS_CHECK_ARG(w && prep, "%s: null pointer", what);
  SplitPrep sp;
  YS_CHECK_ARG(split_prep_carve(prep, prep_bytes, (size_t)2 * cout * cin_pad * TAPS, &sp),
               "%s: block too small (%zu)", what, prep_bytes);
  hipStream_t st = (hipStream_t)stream;
  YS_CHECK_ARG(hipMemsetAsync(sp.flag, 0, sizeof(unsigned), st) == hipSuccess, "%s: flag reset failed", what);
  const long n = (long)cout * cin_pad * TAPS;
  hipLaunchKernelGGL(split_prep_kernel<TAPS>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w, cin, cin_pad,
                     cout, sp.wp, range_flag_dev(), sp.flag);
  YS_CHECK_LAUNCH(what);
  return 0;
}

// Workgroups of a persistent kernel with `slots` resident workgroups on the device and `items` work items: a multiple
// of 8 (workgroup i runs on XCD i % 8, and every XCD walks its own contiguous range of the items), at most one per
// item.
inline long persistent_grid(long slots, long items) {
  const long cap = (items + 7) / 8 * 8;
  return ((slots < cap ? slots : cap) + 7) / 8 * 8;
}

// The tile geometry (of three, tw[g] x th[g] pixels, blk[g] MFMA blocks of work per tile, useful or not) that covers
// an H x W map with the least work; geometry 0 on a tie and for every map above 40 x 40.
inline int pick_geo(int H, int W, const int tw[3], const int th[3], const int blk[3]) {
  if ((long)H * W > 1600) return 0;
  int best = 0;
  long nbest = 0;
  for (int g = 0; g < 3; ++g) {
    const long n = (long)((W + tw[g] - 1) / tw[g]) * ((H + th[g] - 1) / th[g]) * blk[g];
    if (g == 0 || n < nbest) best = g, nbest = n;
  }
  return best;
}

}  // namespace ys
