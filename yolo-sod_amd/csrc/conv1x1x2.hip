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
#include "common.h"

namespace ys {
namespace c1 {

constexpr float WSC = 64.0f;
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

// NP pixels per tile (64 or 128: the weights are read from L2 once per tile, 128 halves that traffic)
// CPW: 16-channel output blocks per wave (2: workgroups of 128 output channels; 4: of 256; 1: of 64, for Cout 64)
// DB: the staged planes are double-buffered (one barrier per stage)
template <bool DUAL, int NP, int CPW = 2, bool DB = false>
__global__ __launch_bounds__(NT, 2) void conv1x1_x2_kernel(Args p) {
  constexpr int PL = NP * PS;           // plane (halves)
  constexpr int NITEM = (KS / 4) * NP;  // (channel quad, pixel) items per stage
  constexpr int NIT = NITEM / NT;
  constexpr int NPB = NP / 16;          // pixel blocks
  static_assert(NITEM % NT == 0, "items");
  __shared__ __attribute__((aligned(16))) h16_t Pl[(DB ? 4 : 2) * PL];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, g = lane >> 4;
  const int ngrp = p.cout / (64 * CPW);
  const int grp = blockIdx.x % ngrp, tile = (blockIdx.x / ngrp) % p.ntile, b = blockIdx.x / (ngrp * p.ntile);
  const int HW = p.HW, p0 = tile * NP, nst = (p.cin + KS - 1) / KS, nks = nst * (KS / 32);  // weights padded to KS
  float rng = 0.f;

  auto rsrc = [&](const void* base, unsigned bytes) {
    const unsigned long long a = (unsigned long long)base;
    return __builtin_amdgcn_make_buffer_rsrc(
        (void*)(((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(a >> 32)) << 32) |
                (unsigned)__builtin_amdgcn_readfirstlane((unsigned)a)),
        (short)0, __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
  };
  // the part of a virtual concat a stage reads (stages from k1 / KS on: x2) as a buffer resource built from scalars
  // per stage (a select between two resource values is lowered to VGPRs, and every load then runs a waterfall loop)
  const float* xb1 = p.x + (long)b * p.xbs;
  const float* xb2 = p.x2 ? p.x2 + (long)b * p.x2bs : xb1;
  // the first part's plane: HW floats, or the HW / 4 of the quarter-size source it is the nearest 2x upsample of
  const int HW1 = p.up_w ? HW >> 2 : HW;
  const unsigned nb1 = (unsigned)((long)p.k1 * HW1 * 4), nb2 = (unsigned)((long)(p.cin - p.k1) * HW * 4);
  const __amdgpu_buffer_rsrc_t rw = rsrc(p.wp, (unsigned)((long)nks * (p.cout >> 4) * 2 * 1024));

  // staging item e = tid + NT i: channel quad e / NP = q0 + (NT / NP) i (channels 4 quad .. + 3 of the stage), pixel
  // e % NP = tid % NP (clamped to the image: pixels past HW load the last pixel, their outputs are not stored)
  static_assert(NT % NP == 0, "a thread stages one pixel");
  const int q0 = tid / NP;
  const int pc = min(p0 + tid % NP, HW - 1);
  int pc1 = pc;  // the pixel's offset in a first-part plane: its source pixel (y >> 1, x >> 1) when that part is upsampled
  if (p.up_w) {
    const int yy = pc / p.up_w, xx = pc - yy * p.up_w;
    pc1 = (yy >> 1) * (p.up_w >> 1) + (xx >> 1);
  }
  f32x4 sv[NIT];
  // the stage / channel offset is in the per-lane offset, so the buffer range check covers it: channels past Cin
  // (the last stage of a Cin that is not a multiple of KS) read 0, as do the padded weights they meet
  auto load_part = [&](int st, int k0, int k1, bool live) __attribute__((always_inline)) {
    const bool second = KS * st >= p.k1;  // stage-uniform
    const int chs = second ? HW : HW1;    // plane stride of the part (scalar)
    const unsigned sx = (unsigned)((second ? KS * st - p.k1 : KS * st) * chs * 4);
    const unsigned vo = (unsigned)((4 * q0 * chs + (second ? pc : pc1)) * 4);
    // !live: an empty range (the last stage's "next stage" loads return 0 at once)
    const __amdgpu_buffer_rsrc_t r = rsrc(second ? xb2 : xb1, live ? (second ? nb2 : nb1) : 0u);
#pragma unroll
    for (int k = 0; k < 4 * NIT; ++k)
      if (k >= k0 && k < k1)
        sv[k >> 2][k & 3] = __builtin_bit_cast(
            float, __builtin_amdgcn_raw_buffer_load_b32(
                       r, vo + sx + (unsigned)((4 * (NT / NP) * (k >> 2) + (k & 3)) * chs * 4), 0, 0));
  };
  // weight fragments of k step s (global), channel blocks cb0 + u, planes 0 / 1
  const int cb0 = grp * 4 * CPW + CPW * wid;
  auto wfrag = [&](int s, int u, int pl) __attribute__((always_inline)) {
    const int st = __builtin_amdgcn_readfirstlane((s * (p.cout >> 4) * 2) * 1024);
    return __builtin_bit_cast(f16x8_t, __builtin_amdgcn_raw_buffer_load_b128(
                                           rw, (unsigned)((((cb0 + u) * 2 + pl) * 64 + lane) * 16), st, 0));
  };
  f32x4 acc[CPW][NPB];
#pragma unroll
  for (int u = 0; u < CPW; ++u)
#pragma unroll
    for (int k = 0; k < NPB; ++k) acc[u][k] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bo[CPW];  // loaded before the loop: an epilogue load would wait behind every load in flight
#pragma unroll
  for (int u = 0; u < CPW; ++u) bo[u] = p.bias[16 * (cb0 + u) + l15];

  // the loaded stage, split, as the two planes at pl
  auto stage_store = [&](h16_t* pl) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int e = tid + NT * i, quad = e / NP, px = e - quad * NP;
      uint2 hh, ll;
      split4x(sv[i], hh, ll);
      rng = range_acc(rng, sv[i]);
      h16_t* d = pl + px * PS + 4 * quad;
      *reinterpret_cast<uint2*>(d) = hh;
      *reinterpret_cast<uint2*>(d + PL) = ll;
    }
  };
  load_part(0, 0, 4 * NIT, true);
  if (DB) {
    stage_store(Pl);
    __syncthreads();
  }
  for (int st = 0; st < nst; ++st) {
    // DB: stage st is in plane pair st & 1 (written during stage st - 1, behind that stage's barrier)
    const h16_t* cur = DB ? Pl + (st & 1) * 2 * PL : Pl;
    if (!DB) {
      __syncthreads();  // every wave is done with the previous stage's planes
      stage_store(Pl);
      __syncthreads();
    }
    const bool nlive = st + 1 < nst;
    const int stn = nlive ? st + 1 : st;
    f16x8_t wa[CPW][2], wn[CPW][2];
#pragma unroll
    for (int u = 0; u < CPW; ++u) {
      wa[u][0] = wfrag(4 * st, u, 0);
      wa[u][1] = wfrag(4 * st, u, 1);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kk = 0; kk < KS / 32; ++kk) {
      const int sn = kk + 1 < KS / 32 ? 4 * st + kk + 1 : 4 * st + kk;  // one k step ahead (unconditional)
#pragma unroll
      for (int u = 0; u < CPW; ++u) {
        wn[u][0] = wfrag(sn, u, 0);
        wn[u][1] = wfrag(sn, u, 1);
      }
      load_part(stn, NIT * kk, NIT * kk + NIT, nlive);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int k = 0; k < NPB; ++k) {
        const h16_t* src = cur + (16 * k + l15) * PS + 32 * kk + 8 * g;
        const f16x8_t xh = *reinterpret_cast<const f16x8_t*>(src);
        const f16x8_t xl = *reinterpret_cast<const f16x8_t*>(src + PL);
#pragma unroll
        for (int u = 0; u < CPW; ++u) {
          f32x4 c = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, wa[u][1], acc[u][k], 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_f16(xl, wa[u][0], c, 0, 0, 0);
          acc[u][k] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, wa[u][0], c, 0, 0, 0);
        }
      }
#pragma unroll
      for (int u = 0; u < CPW; ++u) {
        wa[u][0] = wn[u][0];
        wa[u][1] = wn[u][1];
      }
    }
    if (DB && nlive) {
      // the other pair's last readers were stage st - 1's MFMAs, all done before the barrier that ended that stage;
      // this barrier publishes stage st + 1 and ends the reads of stage st's pair, which stage st + 1 overwrites
      stage_store(Pl + ((st + 1) & 1) * 2 * PL);
      __syncthreads();
    }
  }
  // epilogue: lane (g, l15) of (u, pixel block k) holds channel 16 (cb0 + u) + l15, pixels 16 k + 4 g .. + 3
  float* yb = p.y + (long)b * p.ybs;
#pragma unroll
  for (int u = 0; u < CPW; ++u) {
    const int o = 16 * (cb0 + u) + l15;
#pragma unroll
    for (int k = 0; k < NPB; ++k) {
      const int px = p0 + 16 * k + 4 * g;
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = silu_fast_(acc[u][k][j] * (1.0f / WSC) + bo[u]);
      if (px < HW) {  // HW % 4 == 0: 4 pixels all in or all out
        __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(yb + (long)o * HW + px));
        if (DUAL && o >= p.c2lo)
          __builtin_nontemporal_store(
              v, reinterpret_cast<f32x4*>(p.y2 + (long)b * p.y2bs + (long)(o - p.c2lo) * HW + px));
      }
    }
  }
  range_report(p.range_flag, rng);
  if (p.prep_flag && p.range_flag && blockIdx.x == 0 && threadIdx.x == 0 && *p.prep_flag) *p.range_flag = 1u;
}

// W [Cout][Cin] -> fragment-major planes of 64 W: one thread per (output channel, input channel)
__global__ __launch_bounds__(256) void conv1x1_prep_kernel(const float* __restrict__ w, int cin, int cin_pad,
                                                           int cout, h16_t* __restrict__ wp, unsigned* range_flag,
                                                           unsigned* prep_flag) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)cout * cin_pad) return;
  const int k = (int)(i % cin_pad), n = (int)(i / cin_pad);
  const float v = k < cin ? w[(long)n * cin + k] * WSC : 0.f;  // zero weights for the padded channels
  const _Float16 hh = (_Float16)v;
  const _Float16 ll = (_Float16)(v - (float)hh);
  const int s = k >> 5, kk = k & 31, cbk = n >> 4, ncb = cout >> 4;
  const int ln = ((kk >> 3) << 4) + (n & 15);
  const long base = ((long)(s * ncb + cbk) * 2) * 512 + ln * 8 + (kk & 7);
  wp[base] = __builtin_bit_cast(h16_t, hh);
  wp[base + 512] = __builtin_bit_cast(h16_t, ll);
  const float m = fabsf(v);
  range_report(range_flag, m);
  range_report(prep_flag, m);
}

}  // namespace c1
}  // namespace ys

using namespace ys;

static int c1_pad(int cin) { return (cin + c1::KS - 1) / c1::KS * c1::KS; }

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

static int c1_cu_count() {
  static int n = 0;
  if (n == 0) {
    int dev = 0, c = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0)
      c = 256;
    n = c;
  }
  return n;
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
                         : cout == 512 && HW <= 400 && (long)B * ((HW + 63) / 64) * (cout / 128) > 2L * c1_cu_count();
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
  Sizer s;
  s.take<h16_t>((size_t)2 * cout * c1_pad(cin));
  s.take<unsigned>(1);
  return s.off;
}

static bool c1_carve(void* buf, size_t bytes, int cin, int cout, h16_t** wp, unsigned** flag) {
  Carver cv(buf, bytes);
  *wp = cv.take<h16_t>((size_t)2 * cout * c1_pad(cin));
  *flag = cv.take<unsigned>(1);
  return *flag != nullptr;
}

// Weight preparation (re-run whenever the weights change): w [cout][cin] fp32 (BN folded) -> prep block.
YS_EXPORT int yolosod_conv1x1x2_prepare(const float* w, int cin, int cout, void* prep, size_t prep_bytes,
                                        void* stream) {
  YS_CHECK_ARG(w && prep, "conv1x1x2_prepare: null pointer");
  YS_CHECK_ARG(yolosod_conv1x1x2_prep_bytes(cin, cout) > 0, "conv1x1x2_prepare: (cin=%d, cout=%d) unsupported", cin,
               cout);
  h16_t* wp;
  unsigned* flag;
  YS_CHECK_ARG(c1_carve(prep, prep_bytes, cin, cout, &wp, &flag), "conv1x1x2_prepare: block too small (%zu)",
               prep_bytes);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(flag, 0, sizeof(unsigned), st) != hipSuccess) {
    set_error("conv1x1x2_prepare: flag reset failed");
    return -1;
  }
  const long n = (long)cout * c1_pad(cin);
  hipLaunchKernelGGL(c1::conv1x1_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w, cin, c1_pad(cin),
                     cout, wp, range_flag_dev(), flag);
  YS_CHECK_LAUNCH("conv1x1x2_prep");
  return 0;
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
  h16_t* wp;
  unsigned* flag;
  YS_CHECK_ARG(c1_carve(const_cast<void*>(prep), prep_bytes, cin, cout, &wp, &flag),
               "conv1x1x2: prepared block too small");
  constexpr int NPx = 64;  // pixels per tile (128-pixel tiles measured slower on four of five neck shapes)
  const int ntile = (HW + NPx - 1) / NPx;
  c1::Args a{x, x_bstride, wp, bias, y, y_bstride, y2, y2_bstride, c2lo, cin, cout, HW, ntile, range_flag_dev(), flag,
             x2, x2_bstride, k1, up_w};
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
