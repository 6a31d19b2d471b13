// 1x1 convolution (stride 1, groups 1) + folded BN bias + SiLU on the fp16 matrix cores at fp32 accuracy, for the
// PAN neck's wide 1x1 convs (C2f cv1 / cv2 and the lateral convs of the paper YAML: Cout 128..512, Cin 128..1024;
// ultralytics/nn/modules/conv.py:37-55 with the BN folded by fuse(), block.py:249-253 for C2f's split / concat).
// Per image a GEMM y[Cout][HW] = W[Cout][Cin] x[Cin][HW], epilogue fused: bias, SiLU, the output written into a
// channel slice of a concat buffer, optionally its channels [c2lo, Cout) stored a second time packed (C2f's first
// Bottleneck input). Replaces MIOpen's fp32 GEMM (v_mfma_f32_16x16x4_f32, 157 TF/s) + the separate bias / SiLU pass.
//
// Method as conv3x3.hip: two-term fp16 splits, three v_mfma_f32_16x16x32_f16 per product block, weights x 64 split
// once per parameter version into fragment-major planes (k step s of 32 input channels, 16-channel output block cb,
// plane p: the 64 lanes' fragments are 1 KB contiguous). One 256-thread workgroup per (image, 64-pixel tile, 128
// output channels): per stage of 128 input channels the x tile [128][64] is loaded (4 channels of one pixel per item,
// consecutive threads on consecutive pixels), split and stored as two fp16 planes [pixel][channel] in LDS; wave w
// computes output channel blocks 2 w, 2 w + 1 for the 4 pixel blocks, pixels as the MFMA A operand (a lane holds 4
// consecutive pixels of one channel: 16-byte stores). The next stage's loads are spread over the current stage's
// k steps behind each step's weight prefetch (vmcnt counts in issue order); sched barriers keep them there.
//
// Forms (yolosod_debug_set_conv1x1x2_form; every form adds an output element's products in the same order, so all are
// bit-identical): a wave may own four 16-channel blocks instead of two (workgroups of 256 output channels, Cout % 256
// == 0: the x tile is staged and split once per 256 channels and every pair of LDS reads feeds 12 MFMAs), and the two
// planes may be double-buffered (stage s + 1 is split and written while other waves still run stage s's MFMAs: one
// barrier per stage instead of two, 69632 B of LDS, still two workgroups per CU).
//
// Statistics forms (STATS 1: sum, 2: sum and max; yolosod_conv1x1x2_silu_stats): a conv whose output feeds an SE / CBAM
// gate also emits, per (plane, 64-pixel tile), the sum (and max) of the values exactly as it stores them, from the
// registers the epilogue holds; thin_stats_reduce_kernel (conv_epilogue.hip) adds a plane's tiles in a fixed order
// into the PlaneStats layout the gates read. No atomics: deterministic and independent of the batch size. Everything
// up to the store is the STATS 0 code, so the stored output is bit-identical to it.
#include "split_conv.h"

namespace ys {
namespace c1 {

constexpr float WSC = SPLIT_WSC;
constexpr int KS = 128;        // input channels per stage
constexpr int PS = KS + 8;     // plane row stride (halves): 272-byte pixel rows
constexpr int NT = 256;

struct Args {
  const float* x;      // image b at x + b xbs: [Cin][HW]
  long xbs;
  const h16_t* wp;     // prepared planes
  const float* bias;   // [Cout]
  float* y;            // image b at y + b ybs: [Cout][HW]
  long ybs;
  float* y2;           // optional: channels [c2lo, Cout) again at y2 + b y2bs: [Cout - c2lo][HW]
  long y2bs;
  int c2lo, cin, cout, HW, ntile;
  unsigned* range_flag;
  const unsigned* prep_flag;
  const float* x2;     // optional second input (a virtual concat): channels [k1, Cin) at x2 + b x2bs ([Cin - k1][HW])
  long x2bs;
  int k1;              // channels taken from x (Cin when x2 is NULL; else a multiple of KS)
  int up_w;            // != 0 (with x2): x is the quarter-size source [k1][H/2][up_w/2] of a nearest 2x upsample to
                       // [k1][H][up_w], read in place at (y >> 1, x >> 1)
};
// STATS forms (no second store): y2 = the per-tile partial sums [(b Cout + channel) ntile + tile], y2 + y2bs = the
// partial maxes in the same layout (STATS 2). The struct stays as it is so that the other instances keep their code.

#include "conv1x1x2_kernel.h"
#define YS_C1_STATS_FORMS
#include "conv1x1x2_kernel.h"
#undef YS_C1_STATS_FORMS

}  // namespace c1
}  // namespace ys

using namespace ys;

static int c1_pad(int cin) { return (cin + c1::KS - 1) / c1::KS * c1::KS; }
static size_t c1_halves(int cin, int cout) { return (size_t)2 * cout * c1_pad(cin); }  // of the prepared planes

// Forced form of the kernel (tests / per-shape measurements compare forms; the automatic choice is the product):
// form = groups + 4 buffers; groups 0 automatic, 1 workgroups of 128 output channels, 2 of 256 (Cout % 256 == 0; any
// other Cout runs 1); buffers 0 automatic, 1 one pair of staged planes, 2 two pairs (double-buffered). Cout 64 has one
// form (64-channel workgroups, one pair), reported as 1 + 4 * 1. Returns the previous value.
static int g_c1_form = 0;
YS_EXPORT int yolosod_debug_set_conv1x1x2_form(int form) {
  const int old = g_c1_form;
  if (form >= 0 && form < 12 && (form & 3) != 3) g_c1_form = form;
  return old;
}

// The resolved form (groups 1 .. 2 + 4 * buffers 1 .. 2) of a launch: the forced fields of g_c1_form, the automatic
// choice for the others. Automatic (scripts/bench_conv1x1x2.py forms, batch 32, each library twice):
// 256-channel groups for Cout 512 on maps of at most 20 x 20 when the 128-channel items would not fit the workgroup
// slots (two per CU) in one round - 512 / 768 / 1024 -> 512 at 20^2 run 0.004 - 0.005 ms shorter, more than the
// 0.0035 ms between two runs of one build; at Cout 256 and at 40^2 no form beat the old one by that, and the
// double-buffered forms did nowhere on every shape of a class, so they are forms to force only.
static int c1_form(int B, int cout, int HW) {
  if (cout == 64) return 1 + 4 * 1;
  const int fgrp = g_c1_form & 3, fbuf = g_c1_form >> 2;
  const bool g256 = fgrp ? fgrp == 2
                         : cout == 512 && HW <= 400 && (long)B * ((HW + 63) / 64) * (cout / 128) > 2L * cu_count();
  return (g256 && cout % 256 == 0 ? 2 : 1) + 4 * (fbuf ? fbuf : 1);
}

// The form (as yolosod_debug_set_conv1x1x2_form encodes it, no field 0) a [B][*][H][W] -> cout launch runs in under
// the current setting; 0 for shapes the kernel does not take.
YS_EXPORT int yolosod_debug_conv1x1x2_form(int B, int cout, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || ((long)H * W) % 4 || cout <= 0 || (cout != 64 && cout % 128) || cout > 1024)
    return 0;
  return c1_form(B, cout, H * W);
}

// the 64-pixel-tile instance <dual, 64, CPW, DB> (yolosod_conv1x1x2_silu_cat's NPx)
template <int CPW, bool DB>
static void c1_launch(bool dual, unsigned nwg, hipStream_t st, const c1::Args& a) {
  if (dual) hipLaunchKernelGGL((c1::conv1x1_x2_kernel<true, 64, CPW, DB>), dim3(nwg), dim3(c1::NT), 0, st, a);
  else hipLaunchKernelGGL((c1::conv1x1_x2_kernel<false, 64, CPW, DB>), dim3(nwg), dim3(c1::NT), 0, st, a);
}

// Cout 64 or a multiple of 128 (<= 1024), Cin a multiple of 32 (<= 4096; the weights are padded to a multiple of 128)
YS_EXPORT size_t yolosod_conv1x1x2_prep_bytes(int cin, int cout) {
  if (cin <= 0 || cin % 32 || cin > 4096 || cout <= 0 || (cout != 64 && cout % 128) || cout > 1024) return 0;
  return split_prep_bytes(c1_halves(cin, cout));
}

// Weight preparation (re-run whenever the weights change): w [cout][cin] fp32 (BN folded) -> prep block.
YS_EXPORT int yolosod_conv1x1x2_prepare(const float* w, int cin, int cout, void* prep, size_t prep_bytes,
                                        void* stream) {
  YS_CHECK_ARG(yolosod_conv1x1x2_prep_bytes(cin, cout) > 0, "conv1x1x2_prepare: (cin=%d, cout=%d) unsupported", cin,
               cout);
  return split_prepare<1>("conv1x1x2_prepare", w, cin, c1_pad(cin), cout, prep, prep_bytes, stream);
}

// y = SiLU(W [x; x2] + bias): x image b at x + b x_bstride ([k1][HW]), x2 (or NULL) image b at x2 + b x2_bstride
// ([cin - k1][HW]: the second part of a virtual concat, k1 a multiple of 128), y image b at y + b y_bstride
// ([cout][HW]); y2 (or NULL): channels [c2lo, cout) stored again at y2 + b y2_bstride. HW % 4 == 0; 16-byte aligned
// images. up_w != 0 (with x2): x is the quarter-size source [k1][H/2][up_w/2] of a nearest 2x upsample (the neck's
// nn.Upsample feeding the Concat), read in place at (y >> 1, x >> 1); up_w = the output width W (even, H = HW / W even).
// Same values, staging layout and k order as the materialised form: bit-identical output.
YS_EXPORT int yolosod_conv1x1x2_silu_cat(const float* x, long x_bstride, const float* x2, long x2_bstride, int k1,
                                         float* y, long y_bstride, float* y2, long y2_bstride, int c2lo, int B, int cin,
                                         int cout, int HW, const float* bias, const void* prep, size_t prep_bytes,
                                         int up_w, void* stream) {
  YS_CHECK_ARG(x && y && bias && prep, "conv1x1x2: null pointer");
  if (!x2) k1 = cin;
  YS_CHECK_ARG(up_w == 0 || (x2 && up_w > 0 && up_w % 2 == 0 && HW % up_w == 0 && (HW / up_w) % 2 == 0),
               "conv1x1x2: an upsampled first part needs a second part and even H, W (W=%d, HW=%d)", up_w, HW);
  YS_CHECK_ARG(k1 > 0 && k1 <= cin && (!x2 || (k1 % c1::KS == 0 && k1 < cin && x2_bstride >= (long)(cin - k1) * HW)),
               "conv1x1x2: concat split k1=%d (Cin %d) must be a multiple of %d", k1, cin, c1::KS);
  YS_CHECK_ARG(B >= 0 && HW > 0 && HW % 4 == 0 && yolosod_conv1x1x2_prep_bytes(cin, cout) > 0, "conv1x1x2: bad shape");
  YS_CHECK_ARG(x_bstride >= (long)k1 * (up_w ? HW / 4 : HW) && y_bstride >= (long)cout * HW,
               "conv1x1x2: batch strides too small");
  YS_CHECK_ARG((long)c1_pad(cin) * HW * 4 < (1L << 32), "conv1x1x2: image too large for 32-bit buffer offsets");
  YS_CHECK_ARG((((uintptr_t)y | (uintptr_t)(y2 ? y2 : y)) & 15) == 0 && y_bstride % 4 == 0 && y2_bstride % 4 == 0,
               "conv1x1x2: outputs must be 16-byte aligned");
  YS_CHECK_ARG(!y2 || (c2lo >= 0 && c2lo < cout && y2_bstride >= (long)(cout - c2lo) * HW), "conv1x1x2: c2lo=%d",
               c2lo);
  if (B == 0) return 0;
  SplitPrep sp;
  YS_CHECK_ARG(split_prep_carve(prep, prep_bytes, c1_halves(cin, cout), &sp),
               "conv1x1x2: prepared block too small");
  constexpr int NPx = 64;  // pixels per tile (128-pixel tiles measured slower on four of five neck shapes)
  const int ntile = (HW + NPx - 1) / NPx;
  c1::Args a{x, x_bstride, sp.wp, bias, y, y_bstride, y2, y2_bstride, c2lo, cin, cout, HW, ntile, range_flag_dev(),
             sp.flag, x2, x2_bstride, k1, up_w};
  const int form = c1_form(B, cout, HW);
  const bool g256 = (form & 3) == 2, db = (form >> 2) == 2;
  const long nwg = (long)B * ntile * (cout == 64 ? 1 : cout / (g256 ? 256 : 128));
  YS_CHECK_ARG(nwg < (1L << 31), "conv1x1x2: too many tiles");
  hipStream_t st = (hipStream_t)stream;
  if (cout == 64) c1_launch<1, false>(y2 != nullptr, (unsigned)nwg, st, a);  // a 16-channel block per wave
  else if (g256 && db) c1_launch<4, true>(y2 != nullptr, (unsigned)nwg, st, a);
  else if (g256) c1_launch<4, false>(y2 != nullptr, (unsigned)nwg, st, a);
  else if (db) c1_launch<2, true>(y2 != nullptr, (unsigned)nwg, st, a);
  else c1_launch<2, false>(y2 != nullptr, (unsigned)nwg, st, a);
  YS_CHECK_LAUNCH("conv1x1x2");
  return 0;
}

// y = SiLU(W x + bias) for one input tensor (yolosod_conv1x1x2_silu_cat without a second part)
YS_EXPORT int yolosod_conv1x1x2_silu(const float* x, long x_bstride, float* y, long y_bstride, float* y2,
                                     long y2_bstride, int c2lo, int B, int cin, int cout, int HW, const float* bias,
                                     const void* prep, size_t prep_bytes, void* stream) {
  return yolosod_conv1x1x2_silu_cat(x, x_bstride, nullptr, 0, cin, y, y_bstride, y2, y2_bstride, c2lo, B, cin, cout, HW,
                                    bias, prep, prep_bytes, 0, stream);
}

// yolosod_conv1x1x2_silu (one input, no second store) that also emits the output's per-plane statistics for the SE
// (stats 1: sums) / CBAM (stats 2: sums and maxes) gate that follows, in the psum / pmax[B*cout*parts] layout of
// yolosod_se_forward_pre / yolosod_cbam_forward_pre (parts = yolosod_plane_parts(HW)): k = 0 holds the plane's total,
// k > 0 hold 0 / -inf. tile_ws: 2 * B * cout * ceil(HW / 64) floats. The stored y is bit-identical to
// yolosod_conv1x1x2_silu's. Cout a multiple of 128; the forced group field of yolosod_debug_set_conv1x1x2_form holds,
// the statistics forms have one pair of staged planes.
template <int CPW>
static void c1_launch_stats(int stats, unsigned nwg, hipStream_t st, const c1::Args& a) {
  if (stats == 2)
    hipLaunchKernelGGL((c1::conv1x1_x2s_kernel<CPW, 2>), dim3(nwg), dim3(c1::NT), 0, st, a);
  else
    hipLaunchKernelGGL((c1::conv1x1_x2s_kernel<CPW, 1>), dim3(nwg), dim3(c1::NT), 0, st, a);
}

YS_EXPORT int yolosod_conv1x1x2_silu_stats(const float* x, long x_bstride, float* y, long y_bstride, int B, int cin,
                                           int cout, int HW, const float* bias, const void* prep, size_t prep_bytes,
                                           int stats, int parts, float* psum, float* pmax, float* tile_ws,
                                           void* stream) {
  YS_CHECK_ARG(x && y && bias && prep && psum && tile_ws, "conv1x1x2_stats: null pointer");
  YS_CHECK_ARG((stats == 1 || stats == 2) && (stats == 1 || pmax) && parts >= 1, "conv1x1x2_stats: stats=%d parts=%d",
               stats, parts);
  YS_CHECK_ARG(B >= 0 && HW > 0 && HW % 4 == 0 && cout % 128 == 0 && yolosod_conv1x1x2_prep_bytes(cin, cout) > 0,
               "conv1x1x2_stats: bad shape");
  YS_CHECK_ARG(x_bstride >= (long)cin * HW && y_bstride >= (long)cout * HW, "conv1x1x2_stats: batch strides too small");
  YS_CHECK_ARG((long)c1_pad(cin) * HW * 4 < (1L << 32), "conv1x1x2_stats: image too large for 32-bit buffer offsets");
  YS_CHECK_ARG(((uintptr_t)y & 15) == 0 && y_bstride % 4 == 0, "conv1x1x2_stats: output must be 16-byte aligned");
  if (B == 0) return 0;
  SplitPrep sp;
  YS_CHECK_ARG(split_prep_carve(prep, prep_bytes, c1_halves(cin, cout), &sp),
               "conv1x1x2_stats: prepared block too small");
  const int ntile = (HW + 63) / 64;
  float* tsum = tile_ws;
  float* tmax = tile_ws + (long)B * cout * ntile;
  c1::Args a{x, x_bstride, sp.wp, bias, y, y_bstride, tsum, tmax - tsum, 0, cin, cout, HW, ntile, range_flag_dev(),
             sp.flag, nullptr, 0, cin, 0};
  const bool g256 = (c1_form(B, cout, HW) & 3) == 2;
  const long nwg = (long)B * ntile * (cout / (g256 ? 256 : 128));
  YS_CHECK_ARG(nwg < (1L << 31), "conv1x1x2_stats: too many tiles");
  hipStream_t st = (hipStream_t)stream;
  if (g256) c1_launch_stats<4>(stats, (unsigned)nwg, st, a);
  else c1_launch_stats<2>(stats, (unsigned)nwg, st, a);
  thin_stats_reduce_launch(tsum, stats == 2 ? tmax : nullptr, (long)B * cout, ntile, parts, psum,
                           stats == 2 ? pmax : nullptr, st);
  YS_CHECK_LAUNCH("conv1x1x2_stats");
  return 0;
}
