// 3x3 convolution (stride 1, pad 1, 64 output channels) + folded BN bias + SiLU as an implicit GEMM on the fp16
// matrix cores at fp32 accuracy: the Detect head's conv towers (ultralytics/nn/modules/head.py:
// 43-57: cv2[i] = Conv(c, c2, 3), Conv(c2, c2, 3); cv3[i] = Conv(c, c3, 3), Conv(c3, c3, 3) with c2 = c3 = 64 for the
// paper model). Each Conv is conv2d (no bias) -> BN (folded into weight / bias by fuse(), torch_utils.py:238-265) ->
// SiLU (conv.py:37-55).
//
// Method (the two-term split of swin_x3.hip): v = h + l with h = fp16(v), l = fp16(v - h); a product is
// ah.bh + ah.bl + al.bh on v_mfma_f32_16x16x32_f16 with fp32 accumulation. Weights are split once per parameter
// version by split_prep_kernel (split_conv.h; x 64, exact, so their low terms stay normal fp16) into fragment-major
// planes: for tap t, 32-channel input chunk q, 16-channel output block rb and plane p, the 64 lanes' fragments (lane
// (g, l15): output channel 16 rb + l15, input channels 32 q + 8 g .. + 7) are 1 KB contiguous.
//
// One 256-thread workgroup per (image, 8 x 32 output tile), all 64 output channels, two workgroups per CU: per input
// chunk, the tile's 10 x 34 input halo (zero padding outside the image) is loaded, split and stored once as two fp16
// planes [pixel][32] in LDS; the nine taps read their pixel fragments (8 channels of one halo pixel per lane) at
// tap-shifted pixel offsets of the same planes, so every input value is split once per workgroup and reused by
// 9 taps x 64 outputs. Wave w computes output rows 4 (w >> 1) .. + 3 (eight 16-pixel blocks) for the output channel
// blocks 2 (w & 1), 2 (w & 1) + 1: 16 accumulator tiles from 4 weight fragments (L2, one tap ahead) and 16 pixel
// fragments (LDS) per tap. The pixels are the MFMA's A operand, so a lane's accumulators are 4 consecutive pixels of
// one channel (16-byte stores). The next chunk's halo loads are spread over the current chunk's taps.
#include "split_conv.h"
#include "detect_head_math.h"

namespace ys {
namespace c3 {

constexpr float WSC = SPLIT_WSC;
constexpr int TH = 8, TW = 32;              // output tile
constexpr int HH = TH + 2, HW_ = TW + 2;    // halo tile
constexpr int NPXH = HH * HW_;              // 340 halo pixels
constexpr int PS = 48;                       // plane row stride (halves): 96-byte pixel rows, conflict-free ds_read_b128
constexpr int PL = NPXH * PS;               // plane (halves)
constexpr int NQUAD = NPXH * 8;             // staged items per chunk: (4-channel quad, halo pixel)
constexpr int NT = 256;
constexpr int NIT = (NQUAD + NT - 1) / NT;  // 11

struct Args {
  const float* x;      // [B][Cin][H][W]
  const h16_t* wp;     // prepared planes (fragment-major, x 64)
  const float* bias;   // [Cout]
  float* y;            // image b's output [Cout][H][W] at y + b ybs (a channel slice of a concat buffer when
  long ybs;            // ybs > Cout H W)
  const float* res;    // RES: residual added after the activation (Bottleneck shortcut), image b at res + b rbs
  long rbs;
  int cin, H, W, tiles_x, tiles_y;
  int ncb_all;         // 16-channel blocks of the prepared weights (Cout / 16)
  unsigned* range_flag;
  const unsigned* prep_flag;
  int ntiles;          // persistent kernel: B tiles_y tiles_x
  long xbs;            // image b of x at x + b xbs (>= cin H W: x may be a channel slice of a concat buffer)
};

// conv3x3_head_kernel's arguments: the conv's (y / ybs / res unused) and the head tail's. A type of its own, so that
// the kernels above keep their argument block.
struct HeadTailArgs : Args {
  const h16_t* hw;        // the 1x1 conv's planes (yolosod_detect_head_prepare): hi [t][s][g][row][i], then lo
  const unsigned* hflag;  // their block's range word
  const float* hbias;     // [64] box / [nc] class
  float* hy;              // the level's first anchor of image 0, row 0 of y [B][4 + nc][A]
  long hbs;               // (4 + nc) A
  int A, nc;
  float stride;
};

// One tile per workgroup (the shapes the persistent form below does not take). V4: W % 4 == 0 (16-byte stores).
// CBW: 16-channel blocks per wave (2: output groups of 64 channels; 1: of 32, the neck's C2f at P2), the workgroup's
// group = blockIdx % groups (the groups of a tile run side by side and share its input in L2). RES: + residual.
template <bool V4, int CBW = 2, bool RES = false>
__global__ __launch_bounds__(256, 2) void conv3x3_x2_kernel(Args p) {
  __shared__ __attribute__((aligned(16))) h16_t Pl[2 * PL];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, g = lane >> 4;
  const int ngrp = p.ncb_all / (2 * CBW);
  const int grp = blockIdx.x % ngrp;
  const int t_lin = blockIdx.x / ngrp;
  const int tx = t_lin % p.tiles_x, ty = (t_lin / p.tiles_x) % p.tiles_y, b = t_lin / (p.tiles_x * p.tiles_y);
  const int H = p.H, W = p.W, HWi = H * W;
  const int x0 = tx * TW - 1, y0 = ty * TH - 1;  // halo origin
  const int nq = p.cin >> 5;
  const float* xb = p.x + (long)b * p.xbs;
  float rng = 0.f;

  // staging item e: quad = e / NPXH (channels 4 quad .. + 3 of the chunk), halo pixel e % NPXH; consecutive threads
  // take consecutive pixels (coalesced rows). Out-of-image pixels load a clamped in-image address (unconditional
  // loads) and store zeros. Buffer loads: 32-bit per-lane offsets, the channel / chunk offsets in the scalar offset.
  auto rsrc = [&](const void* base, unsigned bytes) {
    const unsigned long long a = (unsigned long long)base;
    return __builtin_amdgcn_make_buffer_rsrc(
        (void*)(((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(a >> 32)) << 32) |
                (unsigned)__builtin_amdgcn_readfirstlane((unsigned)a)),
        (short)0, __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
  };
  const __amdgpu_buffer_rsrc_t rx = rsrc(xb, (unsigned)((long)p.cin * HWi * 4));
  // the last chunk's "next chunk" loads go through an empty resource: out of range, they return 0 without a memory
  // access (the loads stay unconditional) and no residual / epilogue wait queues behind a needless reload
  const __amdgpu_buffer_rsrc_t rx0 = rsrc(xb, 0u);
  const __amdgpu_buffer_rsrc_t rw = rsrc(p.wp, (unsigned)(9L * nq * p.ncb_all * 2 * 1024));
  unsigned voff[NIT];
  bool okp[NIT];
#pragma unroll
  for (int i = 0; i < NIT; ++i) {
    const int e = min(tid + NT * i, NQUAD - 1);
    const int quad = e / NPXH, px = e - quad * NPXH;
    const int hy = px / HW_, hx = px - hy * HW_;
    const int yy = y0 + hy, xx = x0 + hx;
    okp[i] = yy >= 0 && yy < H && xx >= 0 && xx < W;
    voff[i] = (unsigned)(((4 * quad) * HWi + min(max(yy, 0), H - 1) * W + min(max(xx, 0), W - 1)) * 4);
  }
  f32x4 sv[NIT];
  // loads k = 4 i + c in [k0, k1) of chunk q's staging (item i, channel c of its quad)
  auto load_part = [&](int q, int k0, int k1, bool live) __attribute__((always_inline)) {
    const int sx = __builtin_amdgcn_readfirstlane(32 * q * HWi * 4);
    const __amdgpu_buffer_rsrc_t r = live ? rx : rx0;
#pragma unroll
    for (int k = 0; k < 4 * NIT; ++k)
      if (k >= k0 && k < k1)
        sv[k >> 2][k & 3] = __builtin_bit_cast(
            float, __builtin_amdgcn_raw_buffer_load_b32(r, voff[k >> 2], sx + (k & 3) * HWi * 4, 0));
  };
  auto store_chunk = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int e = tid + NT * i;
      if (e < NQUAD) {
        const int quad = e / NPXH, px = e - quad * NPXH;
        const f32x4 v = okp[i] ? sv[i] : f32x4{0.f, 0.f, 0.f, 0.f};
        uint2 hh, ll;
        split4x(v, hh, ll);
        rng = range_acc(rng, v);
        h16_t* d = Pl + px * PS + 4 * quad;
        *reinterpret_cast<uint2*>(d) = hh;
        *reinterpret_cast<uint2*>(d + PL) = ll;
      }
    }
  };
  // this wave: output channels 32 rp .. + 31 (weight row blocks 2 rp + r), pixel rows 4 ph .. 4 ph + 3 (pixel blocks
  // cb: row 4 ph + (cb >> 1), columns (cb & 1) 16 .. + 15). The pixels are the MFMA's A operand (lane (g, l15) of a
  // fragment: pixel l15 of the block, channels 8 g .. + 7 of the chunk) and the weights its B operand, so the lane
  // holds 4 consecutive pixels (4 g .. + 3) of one output channel (l15): 16-byte output stores
  const int rp = wid & 1, ph = wid >> 1;
  int bpx[8];
#pragma unroll
  for (int cb = 0; cb < 8; ++cb) bpx[cb] = (4 * ph + (cb >> 1)) * HW_ + (cb & 1) * 16 + l15;
  // weight fragments of (tap t, chunk q): channel blocks cbw0 + r (r < CBW), planes 0 / 1; tap t's fragments of chunk
  // q start at byte ((t nq + q) ncb_all 2) KB, [channel block][plane][lane][16 bytes] (B-operand lane layout = A's)
  const int cbw0 = grp * 2 * CBW + CBW * rp;
  auto wfrag = [&](int t, int q, int r, int pl) __attribute__((always_inline)) {
    const int st = __builtin_amdgcn_readfirstlane(((t * nq + q) * p.ncb_all * 2) * 1024);
    return __builtin_bit_cast(f16x8_t, __builtin_amdgcn_raw_buffer_load_b128(
                                           rw, (unsigned)((((cbw0 + r) * 2 + pl) * 64 + lane) * 16), st, 0));
  };
  f32x4 acc[CBW][8];
#pragma unroll
  for (int r = 0; r < CBW; ++r)
#pragma unroll
    for (int cb = 0; cb < 8; ++cb) acc[r][cb] = f32x4{0.f, 0.f, 0.f, 0.f};

  load_part(0, 0, 4 * NIT, true);
  for (int q = 0; q < nq; ++q) {
    __syncthreads();  // every wave is done with the previous chunk's planes
    store_chunk();
    __syncthreads();
    // The next chunk's staging loads are spread over the nine taps, each part issued behind the next tap's weight
    // fragments, and sched barriers keep every prefetch where it is: vmcnt counts in issue order, so a wait for a
    // tap's weights also waits for every halo load issued before them (all 44 at once: the HBM latency at tap 0 of
    // every chunk), and without the barriers the scheduler sinks the loads to their first use (next chunk's staging,
    // next tap) to save registers. Unconditional: the last chunk reloads itself (loads under a branch merge into phis
    // whose copies wait for every load in flight).
    const int qn = q + 1 < nq ? q + 1 : q;
    const bool nlive = q + 1 < nq;
    f16x8_t wa[CBW][2], wn[CBW][2];
#pragma unroll
    for (int r = 0; r < CBW; ++r) {
      wa[r][0] = wfrag(0, q, r, 0);
      wa[r][1] = wfrag(0, q, r, 1);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int tn = t + 1 < 9 ? t + 1 : t;  // one tap ahead (unconditional)
#pragma unroll
      for (int r = 0; r < CBW; ++r) {
        wn[r][0] = wfrag(tn, q, r, 0);
        wn[r][1] = wfrag(tn, q, r, 1);
      }
      load_part(qn, 5 * t, t == 8 ? 4 * NIT : 5 * t + 5, nlive);
      __builtin_amdgcn_sched_barrier(0);
      const int toff = (t / 3) * HW_ + (t % 3);
#pragma unroll
      for (int cb = 0; cb < 8; ++cb) {
        const h16_t* src = Pl + (bpx[cb] + toff) * PS + 8 * g;
        const f16x8_t xh = *reinterpret_cast<const f16x8_t*>(src);
        const f16x8_t xlo = *reinterpret_cast<const f16x8_t*>(src + PL);
#pragma unroll
        for (int r = 0; r < CBW; ++r) {
          // the three split products, small terms first
          f32x4 c = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, wa[r][1], acc[r][cb], 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_f16(xlo, wa[r][0], c, 0, 0, 0);
          acc[r][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, wa[r][0], c, 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < CBW; ++r) {
        wa[r][0] = wn[r][0];
        wa[r][1] = wn[r][1];
      }
    }
  }
  // epilogue: lane (g, l15) of (r, cb) holds output channel 16 (2 rp + r) + l15, pixels (row 4 ph + (cb >> 1),
  // columns (cb & 1) 16 + 4 g .. + 3) of the tile. SiLU on the hardware exp2 / rcp (~2^-22 relative, below the split
  // products' own few-ulp error)
  float* yb = p.y + (long)b * p.ybs;
  float bv[CBW];
#pragma unroll
  for (int r = 0; r < CBW; ++r) bv[r] = p.bias[16 * (cbw0 + r) + l15];
#pragma unroll
  for (int cb = 0; cb < 8; ++cb) {
    const int oy = ty * TH + 4 * ph + (cb >> 1), ox = tx * TW + (cb & 1) * 16 + 4 * g;
#pragma unroll
    for (int r = 0; r < CBW; ++r) {
      const long po = (long)(16 * (cbw0 + r) + l15) * HWi + oy * W + ox;
      float* d = yb + po;
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = silu_fast_(acc[r][cb][j] * (1.0f / WSC) + bv[r]);
      if constexpr (RES) {  // act(conv + b) + x (Bottleneck shortcut, block.py:343); V4 shapes only
#pragma clang fp contract(off)  // a separately rounded add, as x + cv2(...): no fma with SiLU's last multiply
        static_assert(!RES || V4, "residual: W % 4 == 0");
        if (oy < H && ox < W) o = o + *reinterpret_cast<const f32x4*>(p.res + (long)b * p.rbs + po);
      }
      if constexpr (V4) {  // W % 4 == 0: the 4 pixels are all in or all out of the image
        // non-temporal: the tile is not read again before it has left the caches (at P2 the kernel is 13 % faster)
        if (oy < H && ox < W) __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(d));
      } else if (oy < H) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (ox + j < W) d[j] = o[j];
      }
    }
  }
  range_report(p.range_flag, rng);
  if (p.prep_flag && p.range_flag && blockIdx.x == 0 && threadIdx.x == 0 && *p.prep_flag) *p.range_flag = 1u;
}

// Persistent form (W % 4 == 0): the same tile, MFMA and store scheme, but each workgroup walks a contiguous range of
// work items (tile, output group) of its XCD (neighbouring tiles share halo rows in that XCD's L2), one iteration per
// (item, input chunk), and the next iteration's halo loads (the next tile's first chunk included) are spread over the
// current iteration's taps, so no tile starts with an exposed HBM wait. Per-image buffer resources with unclamped
// offsets (rows above the image are negative offsets: out of range, 0); other out-of-image pixels masked by okb.
//
// Geometry G (chosen per launch, c3_pick_geo): a lane holds pixels 4 g .. + 3 of a 16-pixel block, so a block may be
// 16 x 1, 8 x 2 or 4 x 4 pixels (BW x BH) with the same 16-byte stores; a workgroup has 16 block slots (two row-halves
// x 8 per wave) laid out as TBX x TBY blocks (a slot past TBX TBY recomputes block 0 and stores nothing). The order of
// an output element's additions (chunk -> tap -> product) does not depend on G or CBW: every form is bit-identical.
//   G 0: 16 x 1 blocks, 2 x 8: the 32 x 8 tile (P2 / P3), halo 34 x 10
//   G 1:  4 x 4 blocks, 5 x 3: a 20 x 12 tile, halo 22 x 14 (20^2 maps: 78 % of the slots useful against 52 %)
//   G 2:  8 x 2 blocks, 5 x 3: a 40 x 6 tile, halo 42 x 8 (40^2 maps: 89 % against 62.5 %)
// RS: the LDS row stride in pixels. A ds_read_b128 is served in four groups of 16 lanes ({0-3, 12-15, 20-27}, {4-11,
// 16-19, 28-31}, + 32), conflict-free when the group's sixteen 16-byte slots differ mod 16; with 6 slots per pixel
// (PS = 48) a block row must start at slot 8 (mod 16) of the previous one's for 4 x 4 and at slot 0 for 8 x 2:
// RS = 4 (mod 8) >= 22 -> 28, RS = 0 (mod 8) >= 42 -> 48 (tests/test_conv3x3_lds_banks.py enumerates them).
template <int G>
struct Geo;
template <>
struct Geo<0> {
  static constexpr int BW = 16, TBX = 2, TBY = 8, RS = 34;
};
template <>
struct Geo<1> {
  static constexpr int BW = 4, TBX = 5, TBY = 3, RS = 28;
};
template <>
struct Geo<2> {
  static constexpr int BW = 8, TBX = 5, TBY = 3, RS = 48;
};
template <int G>
struct GeoD : Geo<G> {
  using B = Geo<G>;
  static constexpr int BH = 16 / B::BW, NBLK = B::TBX * B::TBY;
  static constexpr int TW = B::TBX * B::BW, TH = B::TBY * BH, HW_ = TW + 2, HH = TH + 2, NPXH = HH * HW_;
  static constexpr int PL = HH * B::RS * PS;  // plane (halves)
  static constexpr int NQUAD = NPXH * 8, NIT = (NQUAD + NT - 1) / NT;
  static_assert(NBLK <= 16 && B::RS >= HW_ && NIT <= 11 && HW_ < 256 && HH < 256, "conv3x3 geometry");
  // wide staging (YS_C3_WIDE_STAGE): items of (quad, halo row, aligned group of four pixels). The NMG groups of a row
  // that start inside the tile give all four pixels; the group before the tile gives its last pixel (halo column 0)
  // and the group after it its first (halo column TW + 1). The whole groups come first, the edge groups after them,
  // so an item's kind is fixed by its place i in the unrolled item loop except in the one place that holds both.
  static constexpr int NMG = TW / 4, NMID = 8 * HH * NMG, NWQ = NMID + 8 * HH * 2, NITW = (NWQ + NT - 1) / NT;
  static_assert(TW % 4 == 0 && NITW <= 4 && TW + 8 < 256, "conv3x3 wide staging");
};

// YS_C3_WIDE_STAGE (diagnostic builds: -DYS_C3_WIDE_STAGE=0 is the staging of one 4-byte load per (channel, halo
// pixel)): the halo is loaded as aligned groups of four pixels, one 16-byte buffer load per channel of a quad. W % 4
// == 0 and 16-byte aligned images make a group lie wholly inside or outside the image row and the buffer range; a
// group past a row's end reads the neighbouring row (in range) or nothing (out of range), and the item's okb bit
// replaces it by zeros. The LDS planes, the split and every MFMA operand are those of the narrow staging.
#ifndef YS_C3_WIDE_STAGE
#define YS_C3_WIDE_STAGE 1
#endif

// The head tail's feature tile (conv3x3_head_kernel): fp32 [pixel][HT_RS] for the tile's 16 blocks of 16 pixels,
// channel c of pixel px at column c ^ ((px & 8) >> 2). With 68-float rows and that swizzle both sides are free of bank
// conflicts (banks of 4 bytes mod 32 per 32-lane half, tests/test_conv3x3_head_isa.py enumerates them): the conv's
// lanes (g, l15) write channel l15 of pixels 4 g .. + 3 (a half holds two g: rows 4 x 68 = 16 banks apart), the tail's
// lanes (g, j) read channels g + 4 q of pixel j (rows 4 banks apart, the swizzle moves pixels 8 .. 15 two banks on).
constexpr int HT_RS = 68;
constexpr int HT_HALVES = 256 * HT_RS * 2;

// F: the wave layout / weight path of a 32-channel output group (CBW == 1; every F is bit-identical, see above).
//   F 0: wave w = (row-half w >> 1: 8 block slots) x (channel block w & 1); weight fragments from L2, one tap ahead.
//   F 1: F 0's layout with the wave's whole weight set (9 taps x 2 planes: 72 VGPRs) loaded once before the item
//        loop. Cin 32 and Cout 32 only (one chunk, one group: the set never changes); the tap loop issues no weight
//        load, so the only vector-memory loads in flight in it are the next iteration's halo.
//   F 2: wave w = block slots 4 w .. 4 w + 3 x both channel blocks: a pixel fragment read from LDS feeds six MFMAs
//        instead of three (8 ds_read_b128 per wave and tap instead of 16); weight fragments from L2, one tap ahead.
// MODE (conv3x3_head_kernel below; 0: none, the kernels of this section): the Detect head's tail in the epilogue, on
// AT = HeadTailArgs.
template <int G, int CBW, bool RES, int F, int MODE = 0, class AT = Args>
__device__ __forceinline__ void conv3x3_p_body(const AT& p) {
  static_assert(F == 0 || CBW == 1, "conv3x3: F 1 / F 2 are forms of the 32-channel group");
  static_assert(MODE == 0 || (F == 0 && CBW == 2 && !RES), "conv3x3: the head tail needs a pixel's 64 channels");
  constexpr int NS = F == 2 ? 4 : 8;    // block slots per wave
  constexpr int CW = F == 2 ? 2 : CBW;  // 16-channel blocks per wave
  using Ge = GeoD<G>;
  constexpr int BW = Ge::BW, BH = Ge::BH, TBX = Ge::TBX, NBLK = Ge::NBLK, RS = Ge::RS;
  constexpr int TH = Ge::TH, TW = Ge::TW, HH = Ge::HH, HW_ = Ge::HW_, NPXH = Ge::NPXH, PL = Ge::PL;
  constexpr bool WIDE = YS_C3_WIDE_STAGE != 0;
  constexpr int NMG = Ge::NMG, NMID = Ge::NMID;
  constexpr int NQUAD = WIDE ? Ge::NWQ : Ge::NQUAD, NIT = WIDE ? Ge::NITW : Ge::NIT;
  // MODE: the planes' memory also holds the tile's fp32 features between the conv and the head tail
  constexpr int PLN = MODE != 0 && HT_HALVES > 2 * PL ? HT_HALVES : 2 * PL;
  __shared__ __attribute__((aligned(16))) h16_t Pl[PLN];
  __shared__ float bsh[512];  // every output channel's bias: an epilogue load would wait behind the prefetches
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, g = lane >> 4;
  const int H = p.H, W = p.W, HWi = H * W, nq = F == 1 ? 1 : p.cin >> 5;
  float rng = 0.f;
  for (int o = tid; o < 16 * p.ncb_all; o += 256) bsh[o] = p.bias[o];  // ordered before use by the loop's barriers
  if constexpr (MODE != 0) {  // the 1x1 conv's bias behind the conv's 64
    if (tid < 64) bsh[64 + tid] = tid < (MODE == 1 ? 64 : p.nc) ? p.hbias[tid] : 0.f;
  }

  const int ngrp = p.ncb_all / (2 * CBW);
  const int nj = gridDim.x >> 3, j = blockIdx.x >> 3, xcd = blockIdx.x & 7;
  const int nitems = p.ntiles * ngrp;
  const int per = (nitems + 7) >> 3;
  const int t_beg = xcd * per + j, t_end = min((xcd + 1) * per, nitems);
  if (t_beg >= t_end) return;
  const int n_it = ((t_end - t_beg + nj - 1) / nj) * nq;

  auto rsrc = [&](const void* base, unsigned bytes) {
    const unsigned long long a = (unsigned long long)base;
    return __builtin_amdgcn_make_buffer_rsrc(
        (void*)(((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(a >> 32)) << 32) |
                (unsigned)__builtin_amdgcn_readfirstlane((unsigned)a)),
        (short)0, __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
  };
  const __amdgpu_buffer_rsrc_t rw = rsrc(p.wp, (unsigned)(9L * nq * p.ncb_all * 2 * 1024));
  __amdgpu_buffer_rsrc_t rhw;
  if constexpr (MODE != 0) rhw = rsrc(p.hw, (unsigned)((MODE == 1 ? 4 : 1) * 4 * 1024));
  int pk[NIT], el0[NIT];
#pragma unroll
  for (int i = 0; i < NIT; ++i) {
    const int e = min(tid + NT * i, NQUAD - 1);
    if constexpr (WIDE) {
      // sixteen consecutive lanes (one lane group of a ds_write_b64) take the 8 quads of two pixel groups: the quads
      // are 8 different bank pairs and the two groups at most a 2-way conflict (whole groups of a geometry start at
      // pixels equal mod 4, that is on the same banks)
      int quad, hy, gx;
      if (e < NMID) {
        const int f = (e >> 4) * 2 + (e & 1);  // pixel group of the tile
        quad = (e >> 1) & 7;
        hy = f / NMG, gx = 4 * (f % NMG);
      } else {
        const int e2 = e - NMID;
        quad = e2 & 7, gx = ((e2 >> 3) & 1) ? TW : -4, hy = e2 >> 4;
      }
      pk[i] = (quad << 16) | (hy << 8) | (gx + 4);
      el0[i] = 4 * quad * HWi + hy * W + gx;
    } else {
      const int quad = e / NPXH, px = e - quad * NPXH;
      const int hy = px / HW_, hx = px - hy * HW_;
      pk[i] = (quad << 16) | (hy << 8) | hx;
      el0[i] = 4 * quad * HWi + hy * W + hx;
    }
  }
  struct It {
    int b, ty, tx, q, grp;
  };
  auto it_of = [&](int it) __attribute__((always_inline)) {
    const int tg = t_beg + (it / nq) * nj;
    const int t = tg / ngrp;
    It r;
    r.grp = tg - t * ngrp;
    r.q = it - (it / nq) * nq;
    r.tx = t % p.tiles_x;
    r.ty = (t / p.tiles_x) % p.tiles_y;
    r.b = t / (p.tiles_x * p.tiles_y);
    return r;
  };
  // narrow: sv[i][0] the item's pixel (4 channels); wide: sv[i][c] the group's four pixels of channel c
  f32x4 sv[NIT][WIDE ? 4 : 1];
  unsigned okb_ld = 0;
  auto load_part = [&](const It& r, int k0, int k1) __attribute__((always_inline)) {
    const int iy0 = TH * r.ty - 1, ix0 = TW * r.tx - (WIDE ? 4 : 1);  // wide: pk's columns count from TW tx - 4
    const __amdgpu_buffer_rsrc_t ri =
        rsrc(p.x + (long)r.b * p.xbs + (long)32 * r.q * HWi, (unsigned)((p.cin - 32 * r.q) * HWi * 4));
    const int toff = iy0 * W + (WIDE ? TW * r.tx : ix0);  // wide: el0's columns count from TW tx
    if (k0 == 0) {
      const bool interior = iy0 >= 0 && ix0 >= 0 && iy0 + HH <= H && TW * r.tx + TW + (WIDE ? 4 : 1) <= W;
      unsigned okb = 0xffffffffu;
      if (!interior) {
        okb = 0;
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
          const int hy = (pk[i] >> 8) & 255, hx = pk[i] & 255;
          okb |= ((unsigned)(iy0 + hy) < (unsigned)H && (unsigned)(ix0 + hx) < (unsigned)W) ? (1u << i) : 0u;
        }
      }
      okb_ld = okb;
    }
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      if (4 * i + 3 < k0 || 4 * i >= k1) continue;
      unsigned vo = (unsigned)((el0[i] + toff) * 4);
      // a masked group (past a ragged tile's image edge: half of the last tile column of an 80-wide map) goes out of
      // the buffer range instead: no memory access for values that are replaced by zeros anyway
      if constexpr (WIDE) vo = ((okb_ld >> i) & 1u) ? vo : 0xfffffff0u;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (4 * i + c >= k0 && 4 * i + c < k1) {
          if constexpr (WIDE)
            sv[i][c] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ri, vo + c * HWi * 4, 0, 0));
          else
            sv[i][0][c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ri, vo + c * HWi * 4, 0, 0));
        }
    }
  };
  // one staged pixel (4 channels of a quad): split, range, the two planes
  auto put = [&](int px, int quad, f32x4 v) __attribute__((always_inline)) {
    uint2 hh, ll;
    split4x(v, hh, ll);
    rng = range_acc(rng, v);
    h16_t* d = Pl + px * PS + 4 * quad;
    *reinterpret_cast<uint2*>(d) = hh;
    *reinterpret_cast<uint2*>(d + PL) = ll;
  };
  const int rp = F == 2 ? 0 : wid & 1, slot0 = F == 2 ? 4 * wid : 8 * (wid >> 1);
  int bpx[NS];
#pragma unroll
  for (int cb = 0; cb < NS; ++cb) {
    const int bi = slot0 + cb < NBLK ? slot0 + cb : 0;  // a slot past the tile's blocks recomputes block 0, unstored
    bpx[cb] = ((bi / TBX) * BH + l15 / BW) * RS + (bi % TBX) * BW + l15 % BW;
  }
  auto wfrag = [&](int t, int q, int cbw, int pl) __attribute__((always_inline)) {
    const int st = __builtin_amdgcn_readfirstlane(((t * nq + q) * p.ncb_all * 2) * 1024);
    return __builtin_bit_cast(f16x8_t, __builtin_amdgcn_raw_buffer_load_b128(
                                           rw, (unsigned)(((cbw * 2 + pl) * 64 + lane) * 16), st, 0));
  };
  f32x4 acc[CW][NS];
#pragma unroll
  for (int r = 0; r < CW; ++r)
#pragma unroll
    for (int cb = 0; cb < NS; ++cb) acc[r][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
  f16x8_t wres[F == 1 ? 9 : 1][2];  // F 1: the wave's weight set (channel block rp of the one group), resident
  if constexpr (F == 1) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      wres[t][0] = wfrag(t, 0, rp, 0);
      wres[t][1] = wfrag(t, 0, rp, 1);
    }
  }
  constexpr int NLD = 4 * NIT;             // loads per (tile, chunk): 16 / 16 / 12 of 16 bytes (narrow: 44 / 40 / 44 of 4)
  constexpr int PER_TAP = (NLD + 8) / 9;   // spread over the nine taps

  It cur = it_of(0);
  load_part(cur, 0, NLD);
  for (int it = 0; it < n_it; ++it) {
    const It r = cur;
    const unsigned okb = okb_ld;
    __syncthreads();  // every wave is done with the previous iteration's planes
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int e = tid + NT * i;
      if (e < NQUAD) {
        const int quad = pk[i] >> 16;
        const bool ok = (okb >> i) & 1u;
        const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (WIDE) {
          // place i of the item loop holds whole groups, edge groups or (one place) both
          const bool all_mid = NT * i + NT <= NMID, all_edge = NT * i >= NMID;  // constants once unrolled
          const bool mid = all_mid || (!all_edge && e < NMID);
          // A place of edge groups only uses one pixel of each 16-byte load. The register allocator then gives the two
          // unused registers of a load's destination to values written while the load is in flight (the next load's
          // address), and the write-after-write wait it needs is a vmcnt(0) inside the tap loop: every halo load in
          // flight, the one just issued included. An empty statement (no instruction) keeps all four registers live.
          if (all_edge) {
#pragma unroll
            for (int c = 0; c < 4; ++c) asm volatile("" : "+v"(sv[i][c]));
          }
          const int g4 = pk[i] & 255;  // 0: the group before the tile (its last pixel is halo column 0)
          const int px = ((pk[i] >> 8) & 255) * RS + max(g4 - 3, 0);
          f32x4 v = f32x4{sv[i][0][0], sv[i][1][0], sv[i][2][0], sv[i][3][0]};
          if (!all_mid && g4 == 0)
            v = f32x4{sv[i][0][3], sv[i][1][3], sv[i][2][3], sv[i][3][3]};
          put(px, quad, ok ? v : z);
          if (mid) {
#pragma unroll
            for (int jx = 1; jx < 4; ++jx)
              put(px + jx, quad, ok ? f32x4{sv[i][0][jx], sv[i][1][jx], sv[i][2][jx], sv[i][3][jx]} : z);
          }
        } else {
          const int px = RS == HW_ ? e - quad * NPXH : ((pk[i] >> 8) & 255) * RS + (pk[i] & 255);
          put(px, quad, ok ? sv[i][0] : z);
        }
      }
    }
    __syncthreads();
    // the last iteration reloads itself (unconditional loads; L2-hot)
    if (it + 1 < n_it) cur = it_of(it + 1);
    const int cbw0 = r.grp * 2 * CBW + CBW * rp;
    f16x8_t wa[CW][2], wn[CW][2];
    if constexpr (F != 1) {
#pragma unroll
      for (int u = 0; u < CW; ++u) {
        wa[u][0] = wfrag(0, r.q, cbw0 + u, 0);
        wa[u][1] = wfrag(0, r.q, cbw0 + u, 1);
      }
    }
    // pixel fragments one (tap, pixel block) step ahead of their MFMAs (across taps too), and group barriers that
    // keep each step's two LDS reads ahead of the previous step's MFMAs: without them the reads sit right before
    // their use and every block waits an LDS round trip
    auto rd = [&](int t, int cb, f16x8_t& h, f16x8_t& l) __attribute__((always_inline)) {
      const h16_t* src = Pl + (bpx[cb] + (t / 3) * RS + (t % 3)) * PS + 8 * g;
      h = *reinterpret_cast<const f16x8_t*>(src);
      l = *reinterpret_cast<const f16x8_t*>(src + PL);
    };
    f16x8_t nh, nl;
    rd(0, 0, nh, nl);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int tn = t + 1 < 9 ? t + 1 : t;
      if constexpr (F != 1) {
#pragma unroll
        for (int u = 0; u < CW; ++u) {
          wn[u][0] = wfrag(tn, r.q, cbw0 + u, 0);
          wn[u][1] = wfrag(tn, r.q, cbw0 + u, 1);
        }
      }
      load_part(cur, PER_TAP * t, min(PER_TAP * t + PER_TAP, NLD));
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int cb = 0; cb < NS; ++cb) {
        const f16x8_t xh = nh, xlo = nl;
        if (cb < NS - 1) rd(t, cb + 1, nh, nl);
        else if (t < 8) rd(t + 1, 0, nh, nl);
#pragma unroll
        for (int u = 0; u < CW; ++u) {
          const f16x8_t w0 = F == 1 ? wres[F == 1 ? t : 0][0] : wa[u][0];
          const f16x8_t w1 = F == 1 ? wres[F == 1 ? t : 0][1] : wa[u][1];
          f32x4 c = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, w1, acc[u][cb], 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_f16(xlo, w0, c, 0, 0, 0);
          acc[u][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, w0, c, 0, 0, 0);
        }
      }
#pragma unroll
      for (int cb = 0; cb < NS; ++cb) {
        if (cb < NS - 1 || t < 8) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // DS read
        __builtin_amdgcn_sched_group_barrier(0x008, 3 * CW, 0);                       // MFMA
      }
      if constexpr (F != 1) {
#pragma unroll
        for (int u = 0; u < CW; ++u) {
          wa[u][0] = wn[u][0];
          wa[u][1] = wn[u][1];
        }
      }
    }
    if constexpr (MODE != 0) {
      // The head's tail instead of the store (detect_head_math.h: detect_head_x2_kernel's arithmetic on the same
      // operands, so the same bits as the store followed by that kernel). The tile's features go through LDS as the
      // fp32 values the store would have written; wave w then takes blocks 4 w .. 4 w + 3 with all 64 channels.
      if (r.q == nq - 1) {
        constexpr int NHT = MODE == 1 ? 4 : 1;  // 16-row output tiles: 4 x 16 DFL bins / the classes
        float bv[CW];
#pragma unroll
        for (int u = 0; u < CW; ++u) bv[u] = bsh[16 * (cbw0 + u) + l15];
#pragma unroll
        for (int cb = 0; cb < NS; ++cb)
#pragma unroll
          for (int u = 0; u < CW; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[u][cb][e] = silu_fast_(acc[u][cb][e] * (1.0f / WSC) + bv[u]);
        __syncthreads();  // every wave is done with the planes
        float* T = reinterpret_cast<float*>(Pl);
#pragma unroll
        for (int cb = 0; cb < NS; ++cb)
#pragma unroll
          for (int u = 0; u < CW; ++u) {
            const int col = (16 * (cbw0 + u) + l15) ^ (g & 2);
#pragma unroll
            for (int e = 0; e < 4; ++e) T[((slot0 + cb) * 16 + 4 * g + e) * HT_RS + col] = acc[u][cb][e];
            acc[u][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
        // the 1x1 conv's fragments, L2-hot, in flight across the barrier (issued once the accumulators'
        // registers are free)
        f16x8_t hwf[NHT * 2][2];
#pragma unroll
        for (int idx = 0; idx < NHT * 2; ++idx)
#pragma unroll
          for (int pl = 0; pl < 2; ++pl)
            hwf[idx][pl] = __builtin_bit_cast(
                f16x8_t, __builtin_amdgcn_raw_buffer_load_b128(
                             rhw, (unsigned)(((pl * NHT * 2 + idx) * 64 + lane) * 16), 0, 0));
        __syncthreads();
        float* yb = p.hy + (long)r.b * p.hbs;
        const int j = l15, sw = (j & 8) >> 2;
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
          const int blk = 4 * wid + k;  // wave-uniform
          if (NBLK < 16 && blk >= NBLK) break;
          const int oy = r.ty * TH + (blk / TBX) * BH + j / BW, ox = r.tx * TW + (blk % TBX) * BW + j % BW;
          const bool ok = oy < H && ox < W;
          const float* tp = T + (blk * 16 + j) * HT_RS;
          float c[16];  // channels g + 4 q of pixel j; a pixel outside the image: zeros, as a load past the level's end
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const float v = tp[(g + 4 * q) ^ sw];
            c[q] = ok ? v : 0.f;
          }
          f32x4 ha[NHT];
#pragma unroll
          for (int t = 0; t < NHT; ++t) ha[t] = f32x4{0.f, 0.f, 0.f, 0.f};
          headm::mma<NHT, 2>(c, [&](int idx, int pl) { return hwf[idx][pl]; }, ha, rng);
          const int pa = oy * W + ox;
          if constexpr (MODE == 1) {
            float bb[4][4], dist[4];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
              for (int e = 0; e < 4; ++e) bb[t][e] = bsh[64 + 16 * t + 4 * g + e];
            headm::dfl(ha, bb, g, dist);
            if (ok) yb[(long)g * p.A + pa] = headm::box_out(dist, ox, oy, p.stride, g);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int c1 = 4 * g + e;
              if (ok && c1 < p.nc) yb[(long)(4 + c1) * p.A + pa] = headm::cls_out(ha[0][e], bsh[64 + c1]);
            }
          }
        }
      }
    } else if (r.q == nq - 1) {
      float* yb = p.y + (long)r.b * p.ybs;
      float bv[CW];
#pragma unroll
      for (int u = 0; u < CW; ++u) bv[u] = bsh[16 * (cbw0 + u) + l15];
#pragma unroll
      for (int cb = 0; cb < NS; ++cb) {
        const int bi = slot0 + cb;
        const int oy = r.ty * TH + (bi / TBX) * BH + (4 * g) / BW, ox = r.tx * TW + (bi % TBX) * BW + (4 * g) % BW;
        const bool live = (NBLK == 16 || bi < NBLK) && oy < H && ox < W;
#pragma unroll
        for (int u = 0; u < CW; ++u) {
          const long po = (long)(16 * (cbw0 + u) + l15) * HWi + oy * W + ox;
          f32x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = silu_fast_(acc[u][cb][e] * (1.0f / WSC) + bv[u]);
          if constexpr (RES) {
#pragma clang fp contract(off)  // a separately rounded add, as x + cv2(...): no fma with SiLU's last multiply
            if (live) o = o + *reinterpret_cast<const f32x4*>(p.res + (long)r.b * p.rbs + po);
          }
          if (live) __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(yb + po));
          acc[u][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
    }
  }
  range_report(p.range_flag, rng);
  if (p.prep_flag && p.range_flag && blockIdx.x == 0 && threadIdx.x == 0 && *p.prep_flag) *p.range_flag = 1u;
  if constexpr (MODE != 0) {
    if (p.hflag && p.range_flag && blockIdx.x == 0 && threadIdx.x == 0 && *p.hflag) *p.range_flag = 1u;
  }
}

template <int G, int CBW, bool RES>
__global__ __launch_bounds__(256, 2) void conv3x3_p_kernel(Args p) {
  conv3x3_p_body<G, CBW, RES, 0>(p);
}

// A Detect tower's last 3x3 conv (64 -> 64) with the tower's 1x1 conv and the decode in its epilogue instead of the
// store: MODE 1 the box tower (64 DFL logits -> cx, cy, w, h of y), MODE 2 the class tower (nc <= 16 logits -> scores).
// The [B, 64, H, W] feature map is never written; the result is bit-identical to conv3x3_p_kernel<G, 2, false>
// followed by detect_head_x2_kernel on that level (the same operands through the same expressions, detect_head_math.h).
template <int G, int MODE>
__global__ __launch_bounds__(256, 2) void conv3x3_head_kernel(HeadTailArgs p) {
  conv3x3_p_body<G, 2, false, 0, MODE, HeadTailArgs>(p);
}

// The F 1 / F 2 forms of the 32-channel group (Cout 32: layer 3's and the neck's P2 Bottleneck convs).
template <int G, bool RES, int F>
__global__ __launch_bounds__(256, 2) void conv3x3_c32_kernel(Args p) {
  conv3x3_p_body<G, 1, RES, F>(p);
}

// ---- The P2 C2f Bottleneck as one launch ----------------------------------------------------------------------------
// y = [res +] SiLU(conv3x3(SiLU(conv3x3(x, W1) + b1), W2) + b2), Cin = Cmid = Cout = 32, stride 1, pad 1, fp32 in and
// out, W % 4 == 0: the two launches of conv3x3_p_kernel<0, 1, *> with the intermediate map kept in LDS instead of
// written to memory and read back (at 160^2 and the bench's batch the pair moves five 105 MB maps, this launch two).
// Bit-identical to the pair: per output element of either conv the additions run tap 0 .. 8, then xh.w1, xl.w0, xh.w0
// on v_mfma_f32_16x16x32_f16, with the same channel-to-k mapping; the epilogue is the pair's expression; the
// intermediate is rounded to fp32, zeroed outside the image (it is the second conv's zero padding, not SiLU(b1)), and
// split with the split4x of the second launch's staging; the shortcut is the exact fp32 input, added separately.
//
// One 512-thread workgroup per CU (157,696 B of LDS), persistent over the 32 x 8 output tiles of its XCD as above:
//   stage   the tile's 12 rows x 40 columns of input (columns 32 tx - 4 .. + 35: ten whole groups of four pixels per
//           row, the 36-wide halo of both convs plus two unused columns each side, so every staged item is a whole
//           group) from registers into two fp16 planes [row][40][PS]; the registers were loaded during the previous
//           tile's first conv;
//   conv 1  on the 10 x 34 intermediate halo taken as 340 consecutive pixels in 22 blocks of 16 (24 slots: 6 per wave
//           quarter, wave w = channel block w & 1 x quarter w >> 1; 24 slots against the 16 of the first launch, so
//           the MFMA work of the pair is x 1.25). The weights are the MFMA's A operand here, so a lane holds four
//           consecutive channels of one pixel and the split intermediate goes to its planes [pixel][PS] with 8-byte
//           stores;
//   conv 2  as conv3x3_p_body (pixels the A operand, four 16 x 1 blocks per wave) from the intermediate planes; the
//           shortcut's loads are issued before its taps, the 16-byte non-temporal stores are the pair's.
// Two barriers per tile: staged input visible / intermediate visible. Weight fragments from L2 through a register ring
// that runs across taps, convs and tiles, five taps ahead (bn_taps). Measured and dropped: fragments one tap
// ahead as in conv3x3_p_body (8 % slower), both channel blocks on every wave (half the LDS reads, twice the weight
// loads: 10 % slower), the second conv's weights resident in registers (no faster).
constexpr int BN_NT = 512;
constexpr int BN_IW = 40, BN_IH = TH + 4;                        // staged input region
constexpr int BN_MW = TW + 2, BN_NM = (TH + 2) * BN_MW;          // intermediate: 34 wide, 340 pixels
constexpr int BN_PL1 = BN_IH * BN_IW * PS, BN_PL2 = BN_NM * PS;  // planes (halves)
constexpr int BN_NQ = 8 * BN_IH * (BN_IW / 4);                   // 960 staged items (quad, row, group of four pixels)
constexpr int BN_NIT = (BN_NQ + BN_NT - 1) / BN_NT;              // 2
constexpr int BN_S1 = 6, BN_S2 = 4;                              // block slots per wave: conv 1 / conv 2
constexpr int BN_LDS = (2 * BN_PL1 + 2 * BN_PL2) * 2 + 64 * 4;
static_assert(4 * BN_S1 * 16 >= BN_NM && BN_LDS <= 160 * 1024, "bottleneck3x3 geometry");

struct BnArgs {
  const float* x;
  long xbs;
  float* y;
  long ybs;
  const float* res;  // RES: the shortcut (the Bottleneck's own input), image b at res + b rbs
  long rbs;
  const h16_t *wp1, *wp2;  // prepared planes of the two convs (yolosod_conv3x3_prepare_ex, 32 -> 32)
  const float *b1, *b2;
  int H, W, tiles_x, tiles_y, ntiles;
  unsigned* range_flag;
  const unsigned *prep_flag1, *prep_flag2;
};

// The nine taps of one conv over NS pixel blocks of this wave (base pixels bpx in planes P, P + PLN of row stride RS):
// pixel fragments one block ahead of their MFMAs (conv3x3_p_body's schedule); per_tap(t) is issued at the head of tap
// t. Weight fragments come from a ring of BN_WD register slots that runs through both convs of every tile (18 tap
// steps per tile, step S0 + t here; the weights do not depend on the tile): step s uses slot s % BN_WD, and the head
// of step s issues wld(step s + BN_WD - 1) into the slot step s - 1 has just finished with, so a fragment is five taps
// in flight and no tap, phase or tile starts on an exposed L2 round trip. WA: the weights as the A operand.
constexpr int BN_WD = 6;
static_assert(18 % BN_WD == 0, "bottleneck3x3: the weight ring's slots are static per tap step");
template <int NS, int RS, int PLN, bool WA, int S0, class WLoad, class PerTap>
__device__ __forceinline__ void bn_taps(const h16_t* P, const int (&bpx)[NS], int g, f16x8_t (&wr)[BN_WD][2],
                                        f32x4 (&acc)[NS], WLoad&& wld, PerTap&& per_tap) {
  auto rd = [&](int t, int cb, f16x8_t& h, f16x8_t& l) __attribute__((always_inline)) {
    const h16_t* src = P + (bpx[cb] + (t / 3) * RS + (t % 3)) * PS + 8 * g;
    h = *reinterpret_cast<const f16x8_t*>(src);
    l = *reinterpret_cast<const f16x8_t*>(src + PLN);
  };
  f16x8_t nh, nl;
  rd(0, 0, nh, nl);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int sn = (S0 + t + BN_WD - 1) % 18;
    wld(sn, wr[sn % BN_WD]);
    per_tap(t);
    __builtin_amdgcn_sched_barrier(0);
    const f16x8_t w0 = wr[(S0 + t) % BN_WD][0], w1 = wr[(S0 + t) % BN_WD][1];
#pragma unroll
    for (int cb = 0; cb < NS; ++cb) {
      const f16x8_t xh = nh, xlo = nl;
      if (cb < NS - 1) rd(t, cb + 1, nh, nl);
      else if (t < 8) rd(t + 1, 0, nh, nl);
      f32x4 c;
      if constexpr (WA) {  // the same three products, small terms first, with the operand roles exchanged
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1, xh, acc[cb], 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0, xlo, c, 0, 0, 0);
        acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0, xh, c, 0, 0, 0);
      } else {
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, w1, acc[cb], 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(xlo, w0, c, 0, 0, 0);
        acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, w0, c, 0, 0, 0);
      }
    }
#pragma unroll
    for (int cb = 0; cb < NS; ++cb) {
      if (cb < NS - 1 || t < 8) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // DS read
      __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);                            // MFMA
    }
  }
}

template <bool RES>
__global__ __launch_bounds__(BN_NT) void bottleneck3x3_c32_kernel(BnArgs p) {
  __shared__ __attribute__((aligned(16))) h16_t Pi[2 * BN_PL1];  // staged input, hi / lo
  __shared__ __attribute__((aligned(16))) h16_t Pm[2 * BN_PL2];  // intermediate, hi / lo
  __shared__ __attribute__((aligned(16))) float bsh[64];         // b1, b2
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, g = lane >> 4;
  const int rp = wid & 1, qt = wid >> 1;  // channel block, quarter of the block slots
  const int H = p.H, W = p.W, HWi = H * W;
  float rng = 0.f;
  if (tid < 64) bsh[tid] = tid < 32 ? p.b1[tid] : p.b2[tid - 32];  // ordered before use by the loop's barriers

  const int nj = gridDim.x >> 3, j = blockIdx.x >> 3, xcd = blockIdx.x & 7;
  const int per = (p.ntiles + 7) >> 3;
  const int t_beg = xcd * per + j, t_end = min((xcd + 1) * per, p.ntiles);
  if (t_beg >= t_end) return;
  const int n_it = (t_end - t_beg + nj - 1) / nj;

  auto rsrc = [&](const void* base, unsigned bytes) {
    const unsigned long long a = (unsigned long long)base;
    return __builtin_amdgcn_make_buffer_rsrc(
        (void*)(((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(a >> 32)) << 32) |
                (unsigned)__builtin_amdgcn_readfirstlane((unsigned)a)),
        (short)0, __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
  };
  const __amdgpu_buffer_rsrc_t rw1 = rsrc(p.wp1, 9u * 4 * 1024), rw2 = rsrc(p.wp2, 9u * 4 * 1024);
  // staging item e: sixteen consecutive lanes take the 8 quads of two pixel groups (conv3x3_p_body's bank layout)
  int pk[BN_NIT], el0[BN_NIT];
#pragma unroll
  for (int i = 0; i < BN_NIT; ++i) {
    const int e = min(tid + BN_NT * i, BN_NQ - 1);
    const int f = (e >> 4) * 2 + (e & 1), quad = (e >> 1) & 7;
    const int hy = f / (BN_IW / 4), gx = 4 * (f % (BN_IW / 4));
    pk[i] = (quad << 16) | (hy << 8) | gx;
    el0[i] = 4 * quad * HWi + hy * W + gx;
  }
  struct It {
    int b, ty, tx;
  };
  auto it_of = [&](int it) __attribute__((always_inline)) {
    const int t = t_beg + it * nj;
    It r;
    r.tx = t % p.tiles_x;
    r.ty = (t / p.tiles_x) % p.tiles_y;
    r.b = t / (p.tiles_x * p.tiles_y);
    return r;
  };
  f32x4 sv[BN_NIT][4];  // sv[i][c]: the group's four pixels of channel c of the item's quad
  unsigned okb_ld = 0;
  auto load_part = [&](const It& r, int k0, int k1) __attribute__((always_inline)) {
    const int iy0 = TH * r.ty - 2, ix0 = TW * r.tx - 4;
    const __amdgpu_buffer_rsrc_t ri = rsrc(p.x + (long)r.b * p.xbs, (unsigned)(32 * HWi * 4));
    const int toff = iy0 * W + ix0;
    if (k0 == 0) {  // W % 4 == 0: a group lies wholly inside or outside the image
      unsigned okb = 0;
#pragma unroll
      for (int i = 0; i < BN_NIT; ++i) {
        const int hy = (pk[i] >> 8) & 255, gx = pk[i] & 255;
        okb |= ((unsigned)(iy0 + hy) < (unsigned)H && (unsigned)(ix0 + gx) < (unsigned)W) ? (1u << i) : 0u;
      }
      okb_ld = okb;
    }
#pragma unroll
    for (int i = 0; i < BN_NIT; ++i) {
      const unsigned vo = ((okb_ld >> i) & 1u) ? (unsigned)((el0[i] + toff) * 4) : 0xfffffff0u;  // masked: no access
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (4 * i + c >= k0 && 4 * i + c < k1)
          sv[i][c] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ri, vo + c * HWi * 4, 0, 0));
    }
  };
  // four channels of one pixel: split, range, the two planes
  auto put = [&](h16_t* P, int pln, int px, int ch, f32x4 v) __attribute__((always_inline)) {
    uint2 hh, ll;
    split4x(v, hh, ll);
    rng = range_acc(rng, v);
    h16_t* d = P + px * PS + ch;
    *reinterpret_cast<uint2*>(d) = hh;
    *reinterpret_cast<uint2*>(d + pln) = ll;
  };
  // conv 1: slot s of this wave is block 6 qt + s of the 340 intermediate pixels, lane pixel m = 16 block + l15 (past
  // the last pixel: pixel 339 again, unstored) at (m / 34, m % 34); its taps start at staged (row, column + 2)
  int bpx1[BN_S1], bpx2[BN_S2];
#pragma unroll
  for (int s = 0; s < BN_S1; ++s) {
    const int m = min(16 * (BN_S1 * qt + s) + l15, BN_NM - 1);
    bpx1[s] = (m / BN_MW) * BN_IW + m % BN_MW + 2;
  }
  // conv 2: block bi = 4 qt + cb is row bi >> 1, columns 16 (bi & 1) .. + 15 of the tile
#pragma unroll
  for (int cb = 0; cb < BN_S2; ++cb) {
    const int bi = BN_S2 * qt + cb;
    bpx2[cb] = (bi >> 1) * BN_MW + (bi & 1) * 16 + l15;
  }
  f32x4 acc1[BN_S1], acc2[BN_S2];
  const f32x4 z4 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < BN_S1; ++s) acc1[s] = z4;
#pragma unroll
  for (int cb = 0; cb < BN_S2; ++cb) acc2[cb] = z4;

  // the weight ring (bn_taps): tap step s of a tile is conv s / 9, tap s % 9; this wave's channel block rp, both planes
  // ([tap][channel block][plane][lane][16 bytes] in a prepared block)
  f16x8_t wr[BN_WD][2];
  auto wld = [&](int step, f16x8_t (&w)[2]) __attribute__((always_inline)) {
    const int st = __builtin_amdgcn_readfirstlane((step % 9) * 4 * 1024);
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
      w[pl] = __builtin_bit_cast(f16x8_t, __builtin_amdgcn_raw_buffer_load_b128(
                                              step < 9 ? rw1 : rw2, (unsigned)(((rp * 2 + pl) * 64 + lane) * 16), st, 0));
  };
#pragma unroll
  for (int s = 0; s < BN_WD - 1; ++s) wld(s, wr[s]);

  It cur = it_of(0);
  load_part(cur, 0, 4 * BN_NIT);
  for (int it = 0; it < n_it; ++it) {
    const It r = cur;
    const unsigned okb = okb_ld;
    // every wave is past the previous tile's second barrier, that is done with its reads of the input planes
#pragma unroll
    for (int i = 0; i < BN_NIT; ++i) {
      if (tid + BN_NT * i < BN_NQ) {
        const int quad = pk[i] >> 16, px = ((pk[i] >> 8) & 255) * BN_IW + (pk[i] & 255);
        const bool ok = (okb >> i) & 1u;
#pragma unroll
        for (int jx = 0; jx < 4; ++jx)
          put(Pi, BN_PL1, px + jx, 4 * quad, ok ? f32x4{sv[i][0][jx], sv[i][1][jx], sv[i][2][jx], sv[i][3][jx]} : z4);
      }
    }
    __syncthreads();  // the staged input is visible; every wave is done with the previous tile's intermediate
    if (it + 1 < n_it) cur = it_of(it + 1);  // the last tile reloads itself (unconditional loads; L2-hot)
    bn_taps<BN_S1, BN_IW, BN_PL1, true, 0>(Pi, bpx1, g, wr, acc1, wld, [&](int t) __attribute__((always_inline)) {
      load_part(cur, t, t + 1);  // the next tile's eight loads, one per tap
    });
    // the intermediate: SiLU(conv + b1) rounded to fp32 as the first launch stored it, zero outside the image, split
    // as the second launch's staging splits what it loads (the empty statement hides the producing multiply from the
    // split's subtraction)
    auto mid = [&](float a, float b, int m) __attribute__((always_inline)) {
      float v = silu_fast_(a * (1.0f / WSC) + b);
      asm volatile("" : "+v"(v));
      const int my = m / BN_MW, mx = m - my * BN_MW;
      const bool in = (unsigned)(TH * r.ty - 1 + my) < (unsigned)H && (unsigned)(TW * r.tx - 1 + mx) < (unsigned)W;
      return in ? v : 0.f;
    };
    // lane: channels 16 rp + 4 g .. + 3 of pixel m (the weights were the A operand)
    const f32x4 b1v = *reinterpret_cast<const f32x4*>(bsh + 16 * rp + 4 * g);
#pragma unroll
    for (int s = 0; s < BN_S1; ++s) {
      const int m = 16 * (BN_S1 * qt + s) + l15;
      const f32x4 v = f32x4{mid(acc1[s][0], b1v[0], m), mid(acc1[s][1], b1v[1], m), mid(acc1[s][2], b1v[2], m),
                            mid(acc1[s][3], b1v[3], m)};
      if (m < BN_NM) put(Pm, BN_PL2, m, 16 * rp + 4 * g, v);
      acc1[s] = z4;
    }
    __syncthreads();  // the intermediate is visible; every wave is done with the input planes
    // the shortcut's loads ahead of the second conv's taps (a masked block goes out of the buffer range)
    const int cho = (16 * rp + l15) * HWi;
    f32x4 rv[BN_S2];
    if constexpr (RES) {
      const __amdgpu_buffer_rsrc_t rr = rsrc(p.res + (long)r.b * p.rbs, (unsigned)(32 * HWi * 4));
#pragma unroll
      for (int cb = 0; cb < BN_S2; ++cb) {
        const int bi = BN_S2 * qt + cb;
        const int oy = r.ty * TH + (bi >> 1), ox = r.tx * TW + (bi & 1) * 16 + 4 * g;
        const unsigned vo = oy < H && ox < W ? (unsigned)((cho + oy * W + ox) * 4) : 0xfffffff0u;
        rv[cb] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rr, vo, 0, 0));
      }
    }
    bn_taps<BN_S2, BN_MW, BN_PL2, false, 9>(Pm, bpx2, g, wr, acc2, wld, [&](int) __attribute__((always_inline)) {});
    float* yb = p.y + (long)r.b * p.ybs;
    const float bv = bsh[32 + 16 * rp + l15];
#pragma unroll
    for (int cb = 0; cb < BN_S2; ++cb) {
      const int bi = BN_S2 * qt + cb;
      const int oy = r.ty * TH + (bi >> 1), ox = r.tx * TW + (bi & 1) * 16 + 4 * g;
      const bool live = oy < H && ox < W;
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = silu_fast_(acc2[cb][e] * (1.0f / WSC) + bv);
      if constexpr (RES) {
#pragma clang fp contract(off)  // a separately rounded add, as x + cv2(...): no fma with SiLU's last multiply
        if (live) o = o + rv[cb];
      }
      if (live) __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(yb + cho + oy * W + ox));
      acc2[cb] = z4;
    }
  }
  range_report(p.range_flag, rng);
  if (p.range_flag && blockIdx.x == 0 && threadIdx.x == 0 &&
      ((p.prep_flag1 && *p.prep_flag1) || (p.prep_flag2 && *p.prep_flag2)))
    *p.range_flag = 1u;
}

}  // namespace c3
}  // namespace ys

using namespace ys;

// Forced form of the persistent kernel (tests / per-shape measurements compare forms; the automatic choice is the
// product): form = geometry + 4 groups; geometry 0 automatic, 1 the 32 x 8 tile, 2 the 20 x 12 tile of 4 x 4 blocks,
// 3 the 40 x 6 tile of 8 x 2 blocks; groups 0 automatic, 1 64-channel output groups, 2 32-channel groups, 3 the
// 32-channel group with the weights resident in registers (F 1: Cin 32 -> Cout 32 only), 4 the 32-channel group with
// both channel blocks on every wave (F 2: Cout 32 only). Every geometry takes every W % 4 == 0 shape; 64-channel
// groups need Cout >= 64. Returns the previous value.
static int g_c3_form = 0;
YS_EXPORT int yolosod_debug_set_conv3x3_form(int form) {
  const int old = g_c3_form;
  if (form >= 0 && form < 20) g_c3_form = form;
  return old;
}

static const int C3_GEO_TW[3] = {c3::GeoD<0>::TW, c3::GeoD<1>::TW, c3::GeoD<2>::TW};
static const int C3_GEO_TH[3] = {c3::GeoD<0>::TH, c3::GeoD<1>::TH, c3::GeoD<2>::TH};

// The geometry with the fewest tiles (every tile is 16 block slots of MFMA work, useful or not) for an H x W map; the
// 32 x 8 tile on a tie and for every map above 40 x 40 (P2 / P3: the form those shapes were tuned on).
static int c3_pick_geo(int H, int W) {
  static const int slots[3] = {16, 16, 16};
  return pick_geo(H, W, C3_GEO_TW, C3_GEO_TH, slots);
}

// The resolved form (geometry 1 .. 3 + 4 * groups 1 .. 2) of a W % 4 == 0 launch: the forced fields of g_c3_form, the
// automatic choice for the others. 32-channel groups (twice the work items, each with half the MFMAs and its own
// staging) when the 64-channel items would leave workgroup slots (two per CU) idle.
// Cin 32 -> Cout 32 (cin 0: not known, as any other Cin) picks among the three forms of the 32-channel group by
// C3_AUTO_C32 (groups field per geometry). Neither new form beat today's on 32 x 32 x 160^2 by more than the
// measurement's spread (resident weights: 0.055 - 0.057 ms against 0.060 - 0.065 plain, 0.069 against 0.068 - 0.073
// with the shortcut; both blocks per wave: 0.065 / 0.073), so none is routed: they are forms to force.
static const int C3_AUTO_C32[3] = {2, 2, 2};
static int c3_form(int B, int cin, int cout, int H, int W) {
  const int fgeo = g_c3_form & 3, fgrp = g_c3_form >> 2;
  const int geo = fgeo ? fgeo - 1 : c3_pick_geo(H, W);
  const long ntiles = (long)B * ((W + C3_GEO_TW[geo] - 1) / C3_GEO_TW[geo]) * ((H + C3_GEO_TH[geo] - 1) / C3_GEO_TH[geo]);
  if (cout == 32) {  // a forced form that does not apply to the shape (resident weights with Cin != 32) resolves to 2
    const int grp = fgrp == 3 ? (cin == 32 ? 3 : 2) : fgrp == 4 ? 4 : fgrp == 0 && cin == 32 ? C3_AUTO_C32[geo] : 2;
    return geo + 1 + 4 * grp;
  }
  const bool g32 = fgrp ? fgrp >= 2 : ntiles * (cout / 64) < 2L * cu_count();
  return geo + 1 + 4 * (g32 ? 2 : 1);
}

static bool c3_cout_ok(int cout) { return cout == 32 || (cout % 64 == 0 && cout <= 512); }

// 3x3 / stride 1 / pad 1 conv with Cout 32 or a multiple of 64 (<= 512): Cin a multiple of 32 (<= 2048)
YS_EXPORT size_t yolosod_conv3x3_prep_bytes_ex(int cin, int cout) {
  if (cin <= 0 || cin % 32 || cin > 2048 || !c3_cout_ok(cout)) return 0;
  return split_prep_bytes((size_t)2 * cout * cin * 9);
}
YS_EXPORT size_t yolosod_conv3x3_prep_bytes(int cin) { return yolosod_conv3x3_prep_bytes_ex(cin, 64); }

// The form (as yolosod_debug_set_conv3x3_form encodes it, no field 0) the persistent kernel runs a [B][*][H][W] ->
// cout launch in under the current setting; 0 for shapes it does not take (W % 4 != 0, unsupported cout).
// The Cin 32 -> Cout 32 forms (groups 3 / 4) are reported by the _ex query, which knows Cin; this one answers for any
// other Cin.
YS_EXPORT int yolosod_debug_conv3x3_form_ex(int B, int cin, int cout, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || W % 4 || !c3_cout_ok(cout)) return 0;
  return c3_form(B, cin, cout, H, W);
}
YS_EXPORT int yolosod_debug_conv3x3_form(int B, int cout, int H, int W) {
  return yolosod_debug_conv3x3_form_ex(B, 0, cout, H, W);
}

// Weight preparation (re-run whenever the weights change): w [cout][cin][3][3] fp32 (BN folded) -> prep block.
YS_EXPORT int yolosod_conv3x3_prepare_ex(const float* w, int cin, int cout, void* prep, size_t prep_bytes,
                                         void* stream) {
  YS_CHECK_ARG(yolosod_conv3x3_prep_bytes_ex(cin, cout) > 0, "conv3x3_prepare: (cin=%d, cout=%d) unsupported", cin,
               cout);
  return split_prepare<9>("conv3x3_prepare", w, cin, cin, cout, prep, prep_bytes, stream);
}
YS_EXPORT int yolosod_conv3x3_prepare(const float* w, int cin, void* prep, size_t prep_bytes, void* stream) {
  return yolosod_conv3x3_prepare_ex(w, cin, 64, prep, prep_bytes, stream);
}

// y = SiLU(conv3x3(x, W) + bias) (+ res): x image b at x + b x_bstride ([cin][H][W]) -> image b's output [cout][H][W] at y + b y_bstride
// (y_bstride >= cout H W: a channel slice of a concat buffer); res (or NULL): image b at res + b res_bstride, added
// after the activation (Bottleneck shortcut). y must not alias x.
YS_EXPORT int yolosod_conv3x3_silu_xs(const float* x, long x_bstride, float* y, long y_bstride, const float* res,
                                      long res_bstride, int B, int cin, int cout, int H, int W, const float* bias,
                                      const void* prep, size_t prep_bytes, void* stream) {
  YS_CHECK_ARG(x && y && bias && prep, "conv3x3: null pointer");
  YS_CHECK_ARG(x_bstride >= (long)cin * H * W, "conv3x3: input batch stride %ld < %ld", x_bstride, (long)cin * H * W);
  YS_CHECK_ARG(B >= 0 && H > 0 && W > 0 && yolosod_conv3x3_prep_bytes_ex(cin, cout) > 0, "conv3x3: bad shape");
  YS_CHECK_ARG((long)cin * H * W < (1L << 31) && (long)cout * H * W < (1L << 31), "conv3x3: plane too large");
  YS_CHECK_ARG(y_bstride >= (long)cout * H * W, "conv3x3: output batch stride %ld < %ld", y_bstride,
               (long)cout * H * W);
  const bool v4 = W % 4 == 0;
  YS_CHECK_ARG(!v4 || (((uintptr_t)y & 15) == 0 && y_bstride % 4 == 0), "conv3x3: output not 16-byte aligned");
  YS_CHECK_ARG(!res || (v4 && ((uintptr_t)res & 15) == 0 && res_bstride % 4 == 0 && res_bstride >= (long)cout * H * W),
               "conv3x3: the residual needs W %% 4 == 0 and 16-byte aligned images");
  if (B == 0) return 0;
  SplitPrep sp;
  YS_CHECK_ARG(split_prep_carve(prep, prep_bytes, (size_t)2 * cout * cin * 9, &sp),
               "conv3x3: prepared block too small");
  c3::Args a{x, sp.wp, bias, y, y_bstride, res, res_bstride, cin, H, W, (W + c3::TW - 1) / c3::TW,
             (H + c3::TH - 1) / c3::TH, cout / 16, range_flag_dev(), sp.flag, 0, x_bstride};
  const int ngrp = cout == 32 ? 1 : cout / 64;
  const long nwg = (long)B * a.tiles_x * a.tiles_y * ngrp;
  YS_CHECK_ARG(nwg < (1L << 31), "conv3x3: too many tiles");
  hipStream_t st = (hipStream_t)stream;
  // the persistent kernel for W % 4 == 0 (two workgroups per CU); the one-tile-per-workgroup kernel otherwise (and
  // for input images that are not 16-byte aligned, which the wide staging's loads need: no tensor of the model)
  const bool x16 = YS_C3_WIDE_STAGE == 0 || (((uintptr_t)x & 15) == 0 && x_bstride % 4 == 0);
  if (v4 && x16) {
    const int fgrp = g_c3_form >> 2;
    YS_CHECK_ARG(!(fgrp == 1 && cout == 32), "conv3x3: 32 outputs have no 64-channel group form");
    const int form = c3_form(B, cin, cout, H, W);
    const int geo = (form & 3) - 1;
    const bool g32 = (form >> 2) >= 2;
    const int fc = (form >> 2) - 2;   // the 32-channel group's F (1 / 2: Cout 32 only, c3_form)
    a.tiles_x = (W + C3_GEO_TW[geo] - 1) / C3_GEO_TW[geo];
    a.tiles_y = (H + C3_GEO_TH[geo] - 1) / C3_GEO_TH[geo];
    a.ntiles = (int)((long)B * a.tiles_x * a.tiles_y);
    const long nitems = (long)a.ntiles * (g32 ? cout / 32 : cout / 64);
    YS_CHECK_ARG(nitems < (1L << 31), "conv3x3: too many tiles");
    const long grid = persistent_grid(2L * cu_count(), nitems);  // two workgroups per CU
    using KP = void (*)(c3::Args);
    static const KP kp[3][2][2] = {
        {{c3::conv3x3_p_kernel<0, 2, false>, c3::conv3x3_p_kernel<0, 2, true>},
         {c3::conv3x3_p_kernel<0, 1, false>, c3::conv3x3_p_kernel<0, 1, true>}},
        {{c3::conv3x3_p_kernel<1, 2, false>, c3::conv3x3_p_kernel<1, 2, true>},
         {c3::conv3x3_p_kernel<1, 1, false>, c3::conv3x3_p_kernel<1, 1, true>}},
        {{c3::conv3x3_p_kernel<2, 2, false>, c3::conv3x3_p_kernel<2, 2, true>},
         {c3::conv3x3_p_kernel<2, 1, false>, c3::conv3x3_p_kernel<2, 1, true>}}};
    static const KP kc[3][2][2] = {
        {{c3::conv3x3_c32_kernel<0, false, 1>, c3::conv3x3_c32_kernel<0, true, 1>},
         {c3::conv3x3_c32_kernel<0, false, 2>, c3::conv3x3_c32_kernel<0, true, 2>}},
        {{c3::conv3x3_c32_kernel<1, false, 1>, c3::conv3x3_c32_kernel<1, true, 1>},
         {c3::conv3x3_c32_kernel<1, false, 2>, c3::conv3x3_c32_kernel<1, true, 2>}},
        {{c3::conv3x3_c32_kernel<2, false, 1>, c3::conv3x3_c32_kernel<2, true, 1>},
         {c3::conv3x3_c32_kernel<2, false, 2>, c3::conv3x3_c32_kernel<2, true, 2>}}};
    const KP k = fc > 0 ? kc[geo][fc - 1][res ? 1 : 0] : kp[geo][g32 ? 1 : 0][res ? 1 : 0];
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(256), 0, st, a);
    YS_CHECK_LAUNCH("conv3x3");
    return 0;
  }
  auto kern = v4 ? c3::conv3x3_x2_kernel<true> : c3::conv3x3_x2_kernel<false>;
  if (cout == 32) {
    kern = res ? c3::conv3x3_x2_kernel<true, 1, true>
               : (v4 ? c3::conv3x3_x2_kernel<true, 1, false> : c3::conv3x3_x2_kernel<false, 1, false>);
  } else if (res) {
    kern = c3::conv3x3_x2_kernel<true, 2, true>;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(256), 0, st, a);
  YS_CHECK_LAUNCH("conv3x3");
  return 0;
}

// As yolosod_conv3x3_silu_xs with a contiguous x [B][cin][H][W].
YS_EXPORT int yolosod_conv3x3_silu_ex(const float* x, float* y, long y_bstride, const float* res, long res_bstride,
                                      int B, int cin, int cout, int H, int W, const float* bias, const void* prep,
                                      size_t prep_bytes, void* stream) {
  return yolosod_conv3x3_silu_xs(x, (long)cin * H * W, y, y_bstride, res, res_bstride, B, cin, cout, H, W, bias, prep,
                                 prep_bytes, stream);
}

// ---- a Detect tower's last conv with the head's tail (64 -> 64 -> decode) -------------------------------------------
// Routing (callers ask yolosod_debug_conv3x3_head_fused; the entry below always runs the fused kernel): automatic (-1)
// fuses a level when its 64 -> 64 launch runs in 64-channel groups (c3_form: at least two workgroup slots per CU worth
// of tiles); a 32-channel group holds half of a pixel's channels and cannot run the tail. 0: never; 1: every shape the
// kernel takes. yolosod_debug_set_conv3x3_head_fuse returns the previous value.
static int g_head_fuse = -1;
YS_EXPORT int yolosod_debug_set_conv3x3_head_fuse(int mode) {
  const int old = g_head_fuse;
  if (mode >= -1 && mode <= 1) g_head_fuse = mode;
  return old;
}

static bool head_tail_shape_ok(int B, int H, int W) {
  return B > 0 && H > 0 && W > 0 && W % 4 == 0 && 64L * H * W * 4 < (1L << 31);
}

YS_EXPORT int yolosod_debug_conv3x3_head_fused(int B, int H, int W) {
  if (!head_tail_shape_ok(B, H, W) || g_head_fuse == 0) return 0;
  return g_head_fuse == 1 || (c3_form(B, 64, 64, H, W) >> 2) == 1;
}

// The box (mode 1) or class (mode 2) tower's tail in one launch: SiLU(conv3x3(x, W) + bias), 64 -> 64, then the
// tower's 1x1 conv (head_prep: yolosod_detect_head_prepare of W [64][64] / [nc][64]; head_bias [64] / [nc]) and the
// decode, into rows 0 .. 3 (mode 1) or 4 .. 4 + nc - 1 (mode 2), anchors a_off .. a_off + H W - 1, of y [B][4 + nc][A].
// Image b of x ([64][H][W], 16-byte aligned) at x + b x_bstride; W % 4 == 0; reg_max 16; 1 <= nc <= 16. The geometry
// is the conv's (the forced field of yolosod_debug_set_conv3x3_form, or the automatic choice); the groups are always
// of 64 channels. Bit-identical to yolosod_conv3x3_silu_xs followed by yolosod_detect_head_levels on that level.
YS_EXPORT int yolosod_conv3x3_head_xs(const float* x, long x_bstride, int B, int H, int W, const float* bias,
                                      const void* prep, size_t prep_bytes, const void* head_prep,
                                      const float* head_bias, int mode, int nc, float stride, float* y, int A, int a_off,
                                      void* stream) {
  YS_CHECK_ARG(x && bias && prep && head_prep && head_bias && y, "conv3x3_head: null pointer");
  YS_CHECK_ARG(mode == 1 || mode == 2, "conv3x3_head: mode=%d (1 box, 2 class)", mode);
  YS_CHECK_ARG(nc >= 1 && nc <= 16, "conv3x3_head: nc=%d unsupported (1..16)", nc);
  YS_CHECK_ARG(B >= 0 && H > 0 && W > 0 && W % 4 == 0, "conv3x3_head: bad shape (W %% 4 == 0 only)");
  YS_CHECK_ARG(64L * H * W * 4 < (1L << 31), "conv3x3_head: plane too large");
  YS_CHECK_ARG(x_bstride >= 64L * H * W && ((uintptr_t)x & 15) == 0 && x_bstride % 4 == 0,
               "conv3x3_head: input images must be 16-byte aligned, batch stride >= %ld", 64L * H * W);
  YS_CHECK_ARG(a_off >= 0 && A > 0 && (long)a_off + (long)H * W <= A, "conv3x3_head: anchors [%d, %ld) outside [0, %d)",
               a_off, (long)a_off + (long)H * W, A);
  YS_CHECK_ARG((long)B * (4 + nc) * A < (1L << 40), "conv3x3_head: output too large");
  if (B == 0) return 0;
  SplitPrep sp, hp;
  YS_CHECK_ARG(split_prep_carve(prep, prep_bytes, (size_t)2 * 64 * 64 * 9, &sp), "conv3x3_head: prepared block too small");
  const size_t hhalves = (size_t)2 * (mode == 1 ? 4 : 1) * 1024;
  split_prep_carve(head_prep, split_prep_bytes(hhalves), hhalves, &hp);
  const int geo = (c3_form(B, 64, 64, H, W) & 3) - 1;
  c3::HeadTailArgs a{};
  a.x = x, a.wp = sp.wp, a.bias = bias, a.cin = 64, a.H = H, a.W = W;
  a.tiles_x = (W + C3_GEO_TW[geo] - 1) / C3_GEO_TW[geo];
  a.tiles_y = (H + C3_GEO_TH[geo] - 1) / C3_GEO_TH[geo];
  a.ncb_all = 4, a.range_flag = range_flag_dev(), a.prep_flag = sp.flag, a.xbs = x_bstride;
  const long ntiles = (long)B * a.tiles_x * a.tiles_y;
  YS_CHECK_ARG(ntiles < (1L << 31), "conv3x3_head: too many tiles");
  a.ntiles = (int)ntiles;
  a.hw = hp.wp, a.hflag = hp.flag, a.hbias = head_bias;
  a.hy = y + a_off, a.hbs = (long)(4 + nc) * A, a.A = A, a.nc = nc, a.stride = stride;
  const long grid = persistent_grid(2L * cu_count(), ntiles);  // two workgroups per CU
  using KH = void (*)(c3::HeadTailArgs);
  static const KH kh[3][2] = {{c3::conv3x3_head_kernel<0, 1>, c3::conv3x3_head_kernel<0, 2>},
                              {c3::conv3x3_head_kernel<1, 1>, c3::conv3x3_head_kernel<1, 2>},
                              {c3::conv3x3_head_kernel<2, 1>, c3::conv3x3_head_kernel<2, 2>}};
  hipLaunchKernelGGL(kh[geo][mode - 1], dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
  YS_CHECK_LAUNCH("conv3x3_head");
  return 0;
}

// ---- the fused Bottleneck (32 -> 32 -> 32) -------------------------------------------------------------------------
// Routing: the pair's intermediate map costs memory traffic only when it does not stay in cache between the two
// launches, so the fused launch is the automatic choice from BN_FUSE_MIN_BYTES of one map (B 32 H W 4) up: the
// smallest size measured (160^2, batches 2 .. 32) from which it beat the pair at every larger one, never below 16 MB
// (DESIGN 24). yolosod_debug_set_bottleneck3x3_fuse: -1 automatic, 0 never, 1 every shape the kernel takes.
static const long BN_FUSE_MIN_BYTES = 8L * 32 * 160 * 160 * 4;
static int g_bn_fuse = -1;
YS_EXPORT int yolosod_debug_set_bottleneck3x3_fuse(int mode) {
  const int old = g_bn_fuse;
  if (mode >= -1 && mode <= 1) g_bn_fuse = mode;
  return old;
}

static bool bn_shape_ok(int B, int H, int W) {
  return B > 0 && H > 0 && W > 0 && W % 4 == 0 && 32L * H * W * 4 < (1L << 31);
}

// Whether a [B][32][H][W] Bottleneck is to run as the fused launch under the current setting (host only).
YS_EXPORT int yolosod_debug_bottleneck3x3_fused(int B, int H, int W) {
  if (!bn_shape_ok(B, H, W) || g_bn_fuse == 0) return 0;
  return g_bn_fuse == 1 || (long)B * 32 * H * W * 4 >= BN_FUSE_MIN_BYTES;
}

// y = [res +] SiLU(conv3x3(SiLU(conv3x3(x, W1) + bias1), W2) + bias2) in one launch, 32 channels throughout, W % 4 == 0,
// bit-identical to yolosod_conv3x3_silu_xs twice: image b of x / y / res ([32][H][W], 16-byte aligned) at x + b
// x_bstride / y + b y_bstride / res + b res_bstride (channel slices of a concat buffer); res NULL: no shortcut; prep1 /
// prep2: the two convs' blocks of yolosod_conv3x3_prepare_ex(w, 32, 32, ...). y must not alias x or res. This entry
// always runs the fused kernel; callers route with yolosod_debug_bottleneck3x3_fused.
YS_EXPORT int yolosod_bottleneck3x3_silu_xs(const float* x, long x_bstride, float* y, long y_bstride, const float* res,
                                            long res_bstride, int B, int H, int W, const float* bias1,
                                            const void* prep1, size_t prep1_bytes, const float* bias2,
                                            const void* prep2, size_t prep2_bytes, void* stream) {
  YS_CHECK_ARG(x && y && bias1 && bias2 && prep1 && prep2, "bottleneck3x3: null pointer");
  YS_CHECK_ARG(B >= 0 && H > 0 && W > 0 && W % 4 == 0, "bottleneck3x3: bad shape (W %% 4 == 0 only)");
  YS_CHECK_ARG(32L * H * W * 4 < (1L << 31), "bottleneck3x3: plane too large");
  const long img = 32L * H * W;
  YS_CHECK_ARG(x_bstride >= img && y_bstride >= img && (!res || res_bstride >= img),
               "bottleneck3x3: batch stride below %ld", img);
  YS_CHECK_ARG(((uintptr_t)x & 15) == 0 && x_bstride % 4 == 0 && ((uintptr_t)y & 15) == 0 && y_bstride % 4 == 0 &&
                   (!res || (((uintptr_t)res & 15) == 0 && res_bstride % 4 == 0)),
               "bottleneck3x3: images not 16-byte aligned");
  if (B == 0) return 0;
  SplitPrep sp1, sp2;
  YS_CHECK_ARG(split_prep_carve(prep1, prep1_bytes, (size_t)2 * 32 * 32 * 9, &sp1) &&
                   split_prep_carve(prep2, prep2_bytes, (size_t)2 * 32 * 32 * 9, &sp2),
               "bottleneck3x3: prepared block too small");
  c3::BnArgs a{x, x_bstride, y, y_bstride, res, res_bstride, sp1.wp, sp2.wp, bias1, bias2, H, W,
               (W + c3::TW - 1) / c3::TW, (H + c3::TH - 1) / c3::TH, 0, range_flag_dev(), sp1.flag, sp2.flag};
  const long ntiles = (long)B * a.tiles_x * a.tiles_y;
  YS_CHECK_ARG(ntiles < (1L << 31), "bottleneck3x3: too many tiles");
  a.ntiles = (int)ntiles;
  const long grid = persistent_grid(cu_count(), ntiles);  // one workgroup per CU (LDS)
  hipStream_t st = (hipStream_t)stream;
  if (res)
    hipLaunchKernelGGL(c3::bottleneck3x3_c32_kernel<true>, dim3((unsigned)grid), dim3(c3::BN_NT), 0, st, a);
  else
    hipLaunchKernelGGL(c3::bottleneck3x3_c32_kernel<false>, dim3((unsigned)grid), dim3(c3::BN_NT), 0, st, a);
  YS_CHECK_LAUNCH("bottleneck3x3");
  return 0;
}

// 3x3 / stride 1 / pad 1 conv with 64 outputs, contiguous y [B][64][H][W].
YS_EXPORT int yolosod_conv3x3_silu(const float* x, float* y, int B, int cin, int H, int W, const float* bias,
                                   const void* prep, size_t prep_bytes, void* stream) {
  return yolosod_conv3x3_silu_ex(x, y, 64L * H * W, nullptr, 0, B, cin, 64, H, W, bias, prep, prep_bytes, stream);
}
