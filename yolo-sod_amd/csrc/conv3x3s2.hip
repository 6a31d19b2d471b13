// 3x3 / stride 2 / pad 1 convolution + folded BN bias + SiLU on the fp16 matrix cores at fp32 accuracy, with the
// channel / spatial gate of the MAFN operator that produces its input applied while the input is staged: the consumer
// of SE_Block L1 (Conv(64, 3, 2) at P1 -> P2) and of CBAM_Block L4 (Conv(256, 3, 2) at P2 -> P3) in the paper YAML
// (cfg yolov12-sod-fusion-v5-simple.yaml rows 1-2 and 4-5). The gate's output y = x * a (SE,
// smallobj_modules.py:92) or y = (x * ca) * sa (CBAM, cbam_block.py:53-54) is formed in registers with exactly the
// reference's fp32 products and goes straight into the convolution (conv.py:37-55 with the BN folded by fuse(),
// torch_utils.py:238-265): the gate's apply pass (read x, write y) and the convolution's re-read of y disappear.
//
// Method as conv3x3.hip: v = h + l fp16 two-term splits, products ah.bh + ah.bl + al.bh on v_mfma_f32_16x16x32_f16,
// weights x 64 split once per parameter version into fragment-major planes (for tap t, 32-channel input chunk q,
// 16-channel output block cb and plane p, the 64 lanes' fragments are 1 KB contiguous).
//
// Two persistent kernels, each workgroup looping over output tiles taken from a contiguous per-XCD range; per tile
// (and 32-channel input chunk) the input halo is staged (gated, split) as two fp16 planes in LDS while the next one's
// loads are in flight in registers. The pixels are the MFMA A operand, so a lane holds 4 consecutive output pixels of
// one channel (16-byte stores).
//   conv3x3s2_rw_kernel: Cout 64 / Cin 32 (the SE L1 -> Conv L2 shape), 32 x 2 output tiles, the weights resident in
//     registers, the output through an LDS tile as 128-byte rows.
//   conv3x3s2_t2_kernel: every other shape, in one of three tile geometries and 64- or 128-channel output groups
//     (s2_form), weight fragments streamed from L2 one tap ahead.
#include "split_conv.h"

namespace ys {
namespace c3s2 {

constexpr float WSC = SPLIT_WSC;
constexpr int TH = 4, TW = 32;              // output tile of the entry's tile-count check; TW: the rw kernel's width
constexpr int HC = 2 * TW + 1;              // input halo columns of a 32-wide tile
constexpr int PS = 32 + 8;                  // plane row stride (halves): stride-2 pixel reads of 16 lanes are 160 B
                                            // apart, which puts the ds_read_b128 lane groups on distinct bank quads

struct Args {
  const float* x;      // [B][Cin][H][W]
  const h16_t* wp;     // prepared planes (fragment-major, x 64)
  const float* bias;   // [Cout]
  const float* gc;     // [B][Cin] channel gate (GATE & 1), 16-byte aligned
  const float* gp;     // [B][H][W] spatial gate (GATE & 2)
  float* y;            // image b's output at y + b ybs: [Cout][Ho][Wo] (ybs >= Cout Ho Wo: a channel slice of a
                       // concat buffer)
  long ybs;
  int B, cin, H, W, Ho, Wo, tiles_x, tiles_y, ntiles;
  int ncb_all;         // channel blocks of the prepared weights (Cout / 16); the t2 kernel: ncb_all / NCB groups
  unsigned* range_flag;
  const unsigned* prep_flag;
};

// Cout 64 / Cin 32 (one input chunk: the SE L1 -> Conv L2 shape): the weights are held in registers for the kernel's
// lifetime (wave w: output channel block w & 3, all taps, 72 VGPRs), so no load but the next tile's input is in flight
// during the taps and all of them are issued right after the staging (no wait for a tap's weights waits behind them);
// wave w computes output rows 2 (w >> 2), + 1 (four pixel blocks) of its 16 channels. The epilogue goes through an
// LDS tile [row][channel][32 px (+4)] and leaves as 128-byte rows (8 lanes per row) while the next tile is staged
// (64-byte lane-group stores straight from the accumulators were store-issue bound).
constexpr int ES = TW + 4;  // epilogue row stride (floats): 144-byte channel rows, conflict-free 16-byte writes
// THk output rows per tile, NTk threads per workgroup (THk = 2, NTk = 256: 72 KB of LDS, two workgroups per CU whose
// staging / compute phases interleave and whose input prefetches are both in flight)
template <int GATE, int THk, int NTk>
__global__ __launch_bounds__(NTk, 512 / NTk) void conv3x3s2_rw_kernel(Args p) {
  constexpr int HRk = 2 * THk + 1, NPXk = HRk * HC, PLk = NPXk * PS, NQUADk = NPXk * 8;
  constexpr int NITk = (NQUADk + NTk - 1) / NTk, NGPk = (NPXk + NTk - 1) / NTk;
  static_assert(NITk <= 32, "okb bits");
  __shared__ __attribute__((aligned(16))) h16_t Pl[2 * PLk];
  __shared__ __attribute__((aligned(16))) float Ep[THk * 64 * ES];
  __shared__ __attribute__((aligned(16))) float gcs[32];
  __shared__ float gps[(GATE & 2) ? NPXk : 1];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, g = lane >> 4;
  const int H = p.H, W = p.W, HWi = H * W;
  const int rp = wid >> 2, cb = wid & 3;  // output rows 2 rp, 2 rp + 1 of the tile; channel block cb
  float rng = 0.f;

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
  const __amdgpu_buffer_rsrc_t rx = rsrc(p.x, 0xffffffffu);
  const __amdgpu_buffer_rsrc_t rw = rsrc(p.wp, (unsigned)(9L * 4 * 2 * 1024));

  // this wave's weights: channel block cb, taps t, planes 0 / 1
  f16x8_t wr[9][2];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
      wr[t][pl] = __builtin_bit_cast(
          f16x8_t, __builtin_amdgcn_raw_buffer_load_b128(rw, (unsigned)(lane * 16), ((t * 4 + cb) * 2 + pl) * 1024, 0));
  // staging item e = tid + NTk i: quad = e / NPXk (channels 4 quad .. + 3), halo pixel e % NPXk = (hy, hx); its element
  // offset in the image for tile origin (0, 0) and its (hy, hx)
  int pk[NITk], el0[NITk];
#pragma unroll
  for (int i = 0; i < NITk; ++i) {
    const int e = min(tid + NTk * i, NQUADk - 1);
    const int quad = e / NPXk, px = e - quad * NPXk;
    const int hy = px / HC, hx = px - hy * HC;
    pk[i] = (quad << 16) | (hy << 8) | hx;
    el0[i] = 4 * quad * HWi + hy * W + hx;
  }
  struct Tile {
    int b, ty, tx;
  };
  auto tile_of = [&](int it) __attribute__((always_inline)) {
    const int t = t_beg + it * nj;
    Tile tl;
    tl.tx = t % p.tiles_x;
    tl.ty = (t / p.tiles_x) % p.tiles_y;
    tl.b = t / (p.tiles_x * p.tiles_y);
    return tl;
  };
  f32x4 sv[NITk];
  float gcv = 0.f, gpv[NGPk];
  unsigned okb_ld = 0;
  // the tile's input: one buffer resource per image (range = the image): offsets of rows above the image are
  // negative (huge as unsigned: out of range, the load returns 0) and every other out-of-image pixel reads some
  // in-image value that okb masks to the zero padding - no clamping on the load path
  auto load_tile = [&](const Tile& tl) __attribute__((always_inline)) {
    const int iy0 = 2 * THk * tl.ty - 1, ix0 = 2 * TW * tl.tx - 1;
    const __amdgpu_buffer_rsrc_t ri = rsrc(p.x + (long)tl.b * 32 * HWi, (unsigned)(32 * HWi * 4));
    const int toff = iy0 * W + ix0;
    const bool interior = iy0 >= 0 && ix0 >= 0 && iy0 + HRk <= H && ix0 + HC <= W;
    unsigned okb = 0xffffffffu;
    if (!interior) {
      okb = 0;
#pragma unroll
      for (int i = 0; i < NITk; ++i) {
        const int hy = (pk[i] >> 8) & 255, hx = pk[i] & 255;
        okb |= ((unsigned)(iy0 + hy) < (unsigned)H && (unsigned)(ix0 + hx) < (unsigned)W) ? (1u << i) : 0u;
      }
    }
#pragma unroll
    for (int i = 0; i < NITk; ++i) {
      const unsigned vo = (unsigned)((el0[i] + toff) * 4);
#pragma unroll
      for (int c = 0; c < 4; ++c)
        sv[i][c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ri, vo + c * HWi * 4, 0, 0));
    }
    okb_ld = okb;
    if constexpr ((GATE & 1) != 0) gcv = p.gc[tl.b * 32 + (tid & 31)];
    if constexpr ((GATE & 2) != 0) {
#pragma unroll
      for (int k = 0; k < NGPk; ++k) {
        const int px = min(tid + NTk * k, NPXk - 1);
        const int hy = px / HC, hx = px - hy * HC;
        gpv[k] = p.gp[(long)tl.b * HWi + min(max(iy0 + hy, 0), H - 1) * W + min(max(ix0 + hx, 0), W - 1)];
      }
    }
  };
  int bpx[4];  // pixel block k: output row 2 rp + (k >> 1), columns (k & 1) 16 .. + 15
#pragma unroll
  for (int k = 0; k < 4; ++k) bpx[k] = 2 * (2 * rp + (k >> 1)) * HC + 2 * ((k & 1) * 16 + l15);
  const int nw = __builtin_amdgcn_readfirstlane(p.Wo);
  const float bo = p.bias[16 * cb + l15];
  // global stores of the epilogue tile: item idx = tid + NTk m: row idx >> 9, channel (idx >> 3) & 63, pixels
  // 4 (idx & 7) .. + 3 (8 lanes per 128-byte row)
  auto store_tile = [&](const Tile& tl) __attribute__((always_inline)) {
#pragma unroll
    for (int m = 0; m < THk * 512 / NTk; ++m) {
      const int idx = tid + NTk * m;
      const int r = idx >> 9, ch = (idx >> 3) & 63, px4 = idx & 7;
      const int ox = tl.tx * TW + 4 * px4, oy = tl.ty * THk + r;
      const f32x4 v = *reinterpret_cast<const f32x4*>(Ep + (r * 64 + ch) * ES + 4 * px4);
      if (oy < p.Ho && ox < nw)
        __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p.y + (long)tl.b * p.ybs + ((long)ch * p.Ho + oy) * nw + ox));
    }
  };

  Tile cur = tile_of(0), prev = cur;
  load_tile(cur);
  for (int it = 0; it < n_it; ++it) {
    const unsigned okb = okb_ld;
    __syncthreads();  // every wave is done with the previous tile's planes, gates and epilogue tile writes
    if constexpr (GATE != 0) {
      if constexpr ((GATE & 1) != 0)
        if (tid < 32) gcs[tid] = gcv;
      if constexpr ((GATE & 2) != 0) {
#pragma unroll
        for (int k = 0; k < NGPk; ++k)
          if (tid + NTk * k < NPXk) gps[tid + NTk * k] = gpv[k];
      }
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < NITk; ++i) {
      const int e = tid + NTk * i;
      if (e < NQUADk) {
        const int quad = pk[i] >> 16, px = e - quad * NPXk;
        f32x4 v = sv[i];
        if constexpr ((GATE & 1) != 0) v = v * *reinterpret_cast<const f32x4*>(gcs + 4 * quad);
        if constexpr ((GATE & 2) != 0) v = v * gps[px];
        if (!((okb >> i) & 1u)) v = f32x4{0.f, 0.f, 0.f, 0.f};
        uint2 hh, ll;
        split4x(v, hh, ll);
        rng = range_acc(rng, v);
        h16_t* d = Pl + px * PS + 4 * quad;
        *reinterpret_cast<uint2*>(d) = hh;
        *reinterpret_cast<uint2*>(d + PLk) = ll;
      }
    }
    // the previous tile's output rows, issued after the staging's waits for this tile's input (a store ahead of
    // them made every wait a full vmcnt(0): the store count under its bounds branch is unknown)
    if (it > 0) store_tile(prev);
    __syncthreads();
    prev = cur;
    if (it + 1 < n_it) cur = tile_of(it + 1);
    load_tile(cur);  // the next tile's input (the last iteration reloads its own): in flight during every tap
    __builtin_amdgcn_sched_barrier(0);
    f32x4 acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int toff = (t / 3) * HC + (t % 3);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const h16_t* src = Pl + (bpx[k] + toff) * PS + 8 * g;
        const f16x8_t xh = *reinterpret_cast<const f16x8_t*>(src);
        const f16x8_t xl = *reinterpret_cast<const f16x8_t*>(src + PLk);
        f32x4 c = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, wr[t][1], acc[k], 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(xl, wr[t][0], c, 0, 0, 0);
        acc[k] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, wr[t][0], c, 0, 0, 0);
      }
    }
    // epilogue tile: lane (g, l15) of pixel block k holds channel 16 cb + l15, pixels (k & 1) 16 + 4 g .. + 3 of
    // row 2 rp + (k >> 1)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = silu_fast_(acc[k][e] * (1.0f / WSC) + bo);
      *reinterpret_cast<f32x4*>(Ep + ((2 * rp + (k >> 1)) * 64 + 16 * cb + l15) * ES + 16 * (k & 1) + 4 * g) = v;
    }
  }
  __syncthreads();
  store_tile(prev);
  range_report(p.range_flag, rng);
  if (p.prep_flag && p.range_flag && blockIdx.x == 0 && threadIdx.x == 0 && *p.prep_flag) *p.range_flag = 1u;
}

// Any (Cout 64 / 128, Cin multiple of 32) with 2-row tiles and 256-thread workgroups, three per CU (LDS 54 KB):
// streamed weights (one tap ahead, the next (tile, chunk)'s input spread over the taps behind them; two per CU at
// Cout 128, whose 8 accumulator tiles per wave need more than 168 registers) with the register-weight kernel's
// unclamped per-image buffer addressing; wave w computes channel blocks
// CBW w .. + CBW - 1 (CBW = NCB / 4) for every pixel block of the tile.
//
// Geometry G (chosen per launch, s2_form): a lane holds output pixels 4 g .. + 3 of a 16-pixel block, so a block may
// be 16 x 1, 8 x 2 or 4 x 4 output pixels (BW x BH) with the same 16-byte stores; a tile is TBX x TBY blocks and every
// wave computes all of them. The order of an output element's additions (chunk -> tap -> product) does not depend on
// G or NCB: every form is bit-identical.
//   G 0: 16 x 1 blocks, 2 x 2: the 32 x 2 tile, input halo 65 x 5 (40-wide outputs: 62.5 % of the MFMAs useful)
//   G 1:  8 x 2 blocks, 5 x 1: a 40 x 2 tile, halo 81 x 5 (40-wide outputs covered exactly)
//   G 2:  4 x 4 blocks, 5 x 1: a 20 x 4 tile, halo 41 x 9 (20-wide outputs covered exactly)
// RS: the LDS row stride in pixels. A ds_read_b128 is served in four groups of 16 lanes ({0-3, 12-15, 20-27}, {4-11,
// 16-19, 28-31}, + 32), conflict-free when the group's sixteen 16-byte slots differ mod 16; with 5 slots per pixel
// (PS = 40) and stride-2 pixel reads a block row must start at slot 0 (mod 16) of the previous one's for 8 x 2 and at
// slot 8 for 4 x 4: RS = 0 (mod 8) >= 81 -> 88, RS = 4 (mod 8) >= 41 -> 44 (tests/test_conv3x3s2_lds_banks.py).
template <int G>
struct Geo;
template <>
struct Geo<0> {
  static constexpr int BW = 16, TBX = 2, TBY = 2, RS = 65;
};
template <>
struct Geo<1> {
  static constexpr int BW = 8, TBX = 5, TBY = 1, RS = 88;
};
template <>
struct Geo<2> {
  static constexpr int BW = 4, TBX = 5, TBY = 1, RS = 44;
};
template <int G>
struct GeoD : Geo<G> {
  using B = Geo<G>;
  static constexpr int BH = 16 / B::BW, NBLK = B::TBX * B::TBY;
  static constexpr int TW = B::TBX * B::BW, TH = B::TBY * BH, HC = 2 * TW + 1, HR = 2 * TH + 1, NPX = HR * HC;
  static constexpr int PL = HR * B::RS * PS;  // plane (halves)
  static constexpr int NQUAD = NPX * 8, NIT = (NQUAD + 255) / 256;
  static_assert(B::RS >= HC && NIT <= 32 && HC < 256 && HR < 256, "conv3x3s2 geometry");
};

// 1: the pixel fragments are read one (tap, pixel block) step ahead of their MFMAs (3 - 5 % per launch on the 5-block
// forms); 0: right before them (the A/B arm of DESIGN §18; its both-gates 40 x 2 instance spills 12 bytes)
#ifndef YS_S2_READ_AHEAD
#define YS_S2_READ_AHEAD 1
#endif

template <int NCB, int GATE, int G>
__global__ __launch_bounds__(256, (NCB == 8 || G != 0) ? 2 : 3) void conv3x3s2_t2_kernel(Args p) {
  using Ge = GeoD<G>;
  constexpr int BW = Ge::BW, BH = Ge::BH, TBX = Ge::TBX, NBLK = Ge::NBLK, RS = Ge::RS;
  constexpr int THk = Ge::TH, TW = Ge::TW, HC = Ge::HC;  // this geometry's, not the 4 x 32 tile's of the file scope
  constexpr int NTk = 256, HRk = Ge::HR, NPXk = Ge::NPX, PLk = Ge::PL, NQUADk = Ge::NQUAD;
  constexpr int NITk = Ge::NIT, NGPk = (NPXk + NTk - 1) / NTk, CBW = NCB / 4;
  static_assert(NCB == 4 || NCB == 8, "Cout 64 or 128");
  // with the read-ahead built in, the three-per-CU instances still keep the fragment reads at their use: the
  // 168-register budget has no room for the fragments in flight (the channel-gated one spilled)
  constexpr bool RA = YS_S2_READ_AHEAD != 0 && !(NCB == 4 && G == 0);
  __shared__ __attribute__((aligned(16))) h16_t Pl[2 * PLk];
  __shared__ __attribute__((aligned(16))) float gcs[32];
  __shared__ float gps[(GATE & 2) ? NPXk : 1];
  __shared__ float bsh[512];  // the bias of every output channel (Cout <= 512): an epilogue load would wait behind
                              // every prefetch in flight
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, g = lane >> 4;
  const int H = p.H, W = p.W, HWi = H * W, nq = p.cin >> 5;
  float rng = 0.f;
  for (int o = tid; o < 16 * p.ncb_all; o += 256) bsh[o] = p.bias[o];  // ordered before use by the loop's barriers

  const int nj = gridDim.x >> 3, j = blockIdx.x >> 3, xcd = blockIdx.x & 7;
  const int ngrp = p.ncb_all / NCB;  // output channel groups of 16 NCB: work item = (tile, group), group fastest
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
  int pk[NITk], el0[NITk];
#pragma unroll
  for (int i = 0; i < NITk; ++i) {
    const int e = min(tid + NTk * i, NQUADk - 1);
    const int quad = e / NPXk, px = e - quad * NPXk;
    const int hy = px / HC, hx = px - hy * HC;
    pk[i] = (quad << 16) | (hy << 8) | hx;
    el0[i] = 4 * quad * HWi + hy * W + hx;
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
  f32x4 sv[NITk];
  float gcv = 0.f, gpv[NGPk];
  unsigned okb_ld = 0;
  // part [k0, k1) of loads k = 4 i + c of (tile, chunk) r: per-image buffer resource (range = the chunk's planes to the
  // image end); rows above the image are negative offsets (out of range: 0), other out-of-image pixels masked by okb
  auto load_part = [&](const It& r, int k0, int k1) __attribute__((always_inline)) {
    const int iy0 = 2 * THk * r.ty - 1, ix0 = 2 * TW * r.tx - 1;
    const __amdgpu_buffer_rsrc_t ri =
        rsrc(p.x + ((long)r.b * p.cin + 32 * r.q) * HWi, (unsigned)((p.cin - 32 * r.q) * HWi * 4));
    const int toff = iy0 * W + ix0;
    if (k0 == 0) {
      const bool interior = iy0 >= 0 && ix0 >= 0 && iy0 + HRk <= H && ix0 + HC <= W;
      unsigned okb = 0xffffffffu;
      if (!interior) {
        okb = 0;
#pragma unroll
        for (int i = 0; i < NITk; ++i) {
          const int hy = (pk[i] >> 8) & 255, hx = pk[i] & 255;
          okb |= ((unsigned)(iy0 + hy) < (unsigned)H && (unsigned)(ix0 + hx) < (unsigned)W) ? (1u << i) : 0u;
        }
      }
      okb_ld = okb;
    }
#pragma unroll
    for (int i = 0; i < NITk; ++i) {
      if (4 * i + 3 < k0 || 4 * i >= k1) continue;
      const unsigned vo = (unsigned)((el0[i] + toff) * 4);
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (4 * i + c >= k0 && 4 * i + c < k1)
          sv[i][c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ri, vo + c * HWi * 4, 0, 0));
    }
  };
  auto load_gates = [&](const It& r) __attribute__((always_inline)) {
    if constexpr ((GATE & 1) != 0) gcv = p.gc[r.b * p.cin + 32 * r.q + (tid & 31)];
    if constexpr ((GATE & 2) != 0) {
      const int iy0 = 2 * THk * r.ty - 1, ix0 = 2 * TW * r.tx - 1;
#pragma unroll
      for (int k = 0; k < NGPk; ++k) {
        const int px = min(tid + NTk * k, NPXk - 1);
        const int hy = px / HC, hx = px - hy * HC;
        gpv[k] = p.gp[(long)r.b * HWi + min(max(iy0 + hy, 0), H - 1) * W + min(max(ix0 + hx, 0), W - 1)];
      }
    }
  };
  auto wfrag = [&](int t, int q, int cb, int pl) __attribute__((always_inline)) {  // cb: over all ncb_all blocks
    const int st = __builtin_amdgcn_readfirstlane((((t * nq + q) * p.ncb_all + cb) * 2 + pl) * 1024);
    return __builtin_bit_cast(f16x8_t, __builtin_amdgcn_raw_buffer_load_b128(rw, (unsigned)(lane * 16), st, 0));
  };
  // pixel block k = (k / TBX, k % TBX) of the tile; the lane's pixel l15 of it = (l15 / BW, l15 % BW): its halo pixel
  // at tap (0, 0) in the plane
  int bpx[NBLK];
#pragma unroll
  for (int k = 0; k < NBLK; ++k) bpx[k] = 2 * ((k / TBX) * BH + l15 / BW) * RS + 2 * ((k % TBX) * BW + l15 % BW);
  f32x4 acc[NBLK][CBW];
#pragma unroll
  for (int k = 0; k < NBLK; ++k)
#pragma unroll
    for (int u = 0; u < CBW; ++u) acc[k][u] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nw = __builtin_amdgcn_readfirstlane(p.Wo);
  constexpr int NLD = 4 * NITk;               // loads per (tile, chunk)
  constexpr int PER_TAP = (NLD + 7) / 8;      // spread over taps 0..7

  It cur = it_of(0);
  load_part(cur, 0, NLD);
  load_gates(cur);
  for (int it = 0; it < n_it; ++it) {
    const It r = cur;
    const unsigned okb = okb_ld;
    __syncthreads();
    if constexpr (GATE != 0) {
      if constexpr ((GATE & 1) != 0)
        if (tid < 32) gcs[tid] = gcv;
      if constexpr ((GATE & 2) != 0) {
#pragma unroll
        for (int k = 0; k < NGPk; ++k)
          if (tid + NTk * k < NPXk) gps[tid + NTk * k] = gpv[k];
      }
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < NITk; ++i) {
      const int e = tid + NTk * i;
      if (e < NQUADk) {
        const int quad = pk[i] >> 16, px = e - quad * NPXk;
        f32x4 v = sv[i];
        if constexpr ((GATE & 1) != 0) v = v * *reinterpret_cast<const f32x4*>(gcs + 4 * quad);
        if constexpr ((GATE & 2) != 0) v = v * gps[px];
        if (!((okb >> i) & 1u)) v = f32x4{0.f, 0.f, 0.f, 0.f};
        uint2 hh, ll;
        split4x(v, hh, ll);
        rng = range_acc(rng, v);
        const int pxl = RS == HC ? px : ((pk[i] >> 8) & 255) * RS + (pk[i] & 255);  // the pixel's place in the plane
        h16_t* d = Pl + pxl * PS + 4 * quad;
        *reinterpret_cast<uint2*>(d) = hh;
        *reinterpret_cast<uint2*>(d + PLk) = ll;
      }
    }
    __syncthreads();
    if (it + 1 < n_it) cur = it_of(it + 1);
    const int cb0 = r.grp * NCB + CBW * wid;  // this wave's first channel block (of all ncb_all)
    f16x8_t wa[CBW][2], wn[CBW][2];
#pragma unroll
    for (int u = 0; u < CBW; ++u) {
      wa[u][0] = wfrag(0, r.q, cb0 + u, 0);
      wa[u][1] = wfrag(0, r.q, cb0 + u, 1);
    }
    // RA: pixel fragments one (tap, pixel block) step ahead of their MFMAs (across taps too), and group barriers that
    // keep each step's two LDS reads ahead of the previous step's MFMAs (as conv3x3_p_kernel); otherwise each block's
    // reads sit right before its MFMAs
    auto rd = [&](int t, int k, f16x8_t& h, f16x8_t& l) __attribute__((always_inline)) {
      const h16_t* src = Pl + (bpx[k] + (t / 3) * RS + (t % 3)) * PS + 8 * g;
      h = *reinterpret_cast<const f16x8_t*>(src);
      l = *reinterpret_cast<const f16x8_t*>(src + PLk);
    };
    f16x8_t nh, nl;
    if constexpr (RA) rd(0, 0, nh, nl);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int tn = t + 1 < 9 ? t + 1 : t;
#pragma unroll
      for (int u = 0; u < CBW; ++u) {
        wn[u][0] = wfrag(tn, r.q, cb0 + u, 0);
        wn[u][1] = wfrag(tn, r.q, cb0 + u, 1);
      }
      if (t < 8) load_part(cur, PER_TAP * t, min(PER_TAP * t + PER_TAP, NLD));
      else load_gates(cur);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int k = 0; k < NBLK; ++k) {
        f16x8_t xh, xl;
        if constexpr (RA) {
          xh = nh, xl = nl;
          if (k < NBLK - 1) rd(t, k + 1, nh, nl);
          else if (t < 8) rd(t + 1, 0, nh, nl);
        } else {
          rd(t, k, xh, xl);
        }
#pragma unroll
        for (int u = 0; u < CBW; ++u) {
          f32x4 c = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, wa[u][1], acc[k][u], 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_f16(xl, wa[u][0], c, 0, 0, 0);
          acc[k][u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, wa[u][0], c, 0, 0, 0);
        }
      }
      if constexpr (RA) {
#pragma unroll
        for (int k = 0; k < NBLK; ++k) {
          if (k < NBLK - 1 || t < 8) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // DS read
          __builtin_amdgcn_sched_group_barrier(0x008, 3 * CBW, 0);                       // MFMA
        }
      }
#pragma unroll
      for (int u = 0; u < CBW; ++u) {
        wa[u][0] = wn[u][0];
        wa[u][1] = wn[u][1];
      }
    }
    if (r.q == nq - 1) {
      float bo[CBW];
#pragma unroll
      for (int u = 0; u < CBW; ++u) bo[u] = bsh[16 * (cb0 + u) + l15];
      f32x4 v[NBLK][CBW];
#pragma unroll
      for (int k = 0; k < NBLK; ++k)
#pragma unroll
        for (int u = 0; u < CBW; ++u)
#pragma unroll
          for (int e = 0; e < 4; ++e) v[k][u][e] = silu_fast_(acc[k][u][e] * (1.0f / WSC) + bo[u]);
      // lane (g, l15) of pixel block k holds channel l15 of its block, pixels 4 g .. + 3 of the block: row (4 g) / BW,
      // columns (4 g) % BW .. + 3
#pragma unroll
      for (int k = 0; k < NBLK; ++k) {
        const int oy = r.ty * THk + (k / TBX) * BH + (4 * g) / BW, ox = r.tx * TW + (k % TBX) * BW + (4 * g) % BW;
#pragma unroll
        for (int u = 0; u < CBW; ++u) {
          const int o = 16 * (cb0 + u) + l15;
          if (oy < p.Ho && ox < nw)
            __builtin_nontemporal_store(
                v[k][u], reinterpret_cast<f32x4*>(p.y + (long)r.b * p.ybs + ((long)o * p.Ho + oy) * nw + ox));
          acc[k][u] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
    }
  }
  range_report(p.range_flag, rng);
  if (p.prep_flag && p.range_flag && blockIdx.x == 0 && threadIdx.x == 0 && *p.prep_flag) *p.range_flag = 1u;
}

}  // namespace c3s2
}  // namespace ys

using namespace ys;

// 3x3 / stride 2 / pad 1 conv with Cout 64 or a multiple of 128 (<= 512) and Cin a multiple of 32 (<= 2048)
YS_EXPORT size_t yolosod_conv3x3s2_prep_bytes(int cin, int cout) {
  if (cin <= 0 || cin % 32 || cin > 2048 || !(cout == 64 || (cout % 128 == 0 && cout <= 512))) return 0;
  return split_prep_bytes((size_t)2 * cout * cin * 9);
}

// Forced form of the tiled kernel (tests / per-shape measurements compare forms; the automatic choice is the
// product): form = geometry + 4 groups; geometry 0 automatic, 1 the 32 x 2 tile, 2 the 40 x 2 tile of 8 x 2 blocks,
// 3 the 20 x 4 tile of 4 x 4 blocks; groups 0 automatic, 1 128-channel output groups, 2 64-channel groups (Cout 64
// has 64-channel groups only, whatever is forced). Every geometry takes every shape. Returns the previous value.
static int g_s2_form = 0;
YS_EXPORT int yolosod_debug_set_conv3x3s2_form(int form) {
  const int old = g_s2_form;
  if (form >= 0 && form < 12) g_s2_form = form;
  return old;
}

static const int S2_GEO_TW[3] = {c3s2::GeoD<0>::TW, c3s2::GeoD<1>::TW, c3s2::GeoD<2>::TW};
static const int S2_GEO_TH[3] = {c3s2::GeoD<0>::TH, c3s2::GeoD<1>::TH, c3s2::GeoD<2>::TH};

// The geometry with the fewest tiles for an Ho x Wo output (the 40 x 2 and 20 x 4 tiles carry 1.25 times a 32 x 2
// tile's MFMA work, useful or not: compared in blocks); the 32 x 2 tile on a tie and for every output above 40 x 40
// (a store's 16 lanes cover 64 contiguous bytes per channel there, 32 or 16 in the other forms).
static int s2_pick_geo(int Ho, int Wo) {
  static const int nblk[3] = {c3s2::GeoD<0>::NBLK, c3s2::GeoD<1>::NBLK, c3s2::GeoD<2>::NBLK};
  return pick_geo(Ho, Wo, S2_GEO_TW, S2_GEO_TH, nblk);
}

// The resolved form (geometry 1 .. 3 + 4 * groups 1 .. 2) of a launch: the forced fields of g_s2_form, the automatic
// choice for the others. 128-channel groups whenever Cout has them (64-channel groups halve the MFMAs per LDS read
// and per weight fragment; measured slower on every model shape).
static int s2_form(int B, int cout, int Ho, int Wo) {
  const int fgeo = g_s2_form & 3, fgrp = (g_s2_form >> 2) & 3;
  const int geo = fgeo ? fgeo - 1 : s2_pick_geo(Ho, Wo);
  const bool g64 = cout == 64 || fgrp == 2;
  return geo + 1 + 4 * (g64 ? 2 : 1);
}

// The form (as yolosod_debug_set_conv3x3s2_form encodes it, no field 0) the tiled kernel runs a [B][*][H][W] -> cout
// launch in under the current setting; 0 for shapes it does not take.
YS_EXPORT int yolosod_debug_conv3x3s2_form(int B, int cout, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || ((W + 1) / 2) % 4 || !(cout == 64 || (cout % 128 == 0 && cout <= 512))) return 0;
  return s2_form(B, cout, (H + 1) / 2, (W + 1) / 2);
}

// Weight preparation (re-run whenever the weights change): w [cout][cin][3][3] fp32 (BN folded) -> prep block.
YS_EXPORT int yolosod_conv3x3s2_prepare(const float* w, int cin, int cout, void* prep, size_t prep_bytes,
                                        void* stream) {
  YS_CHECK_ARG(yolosod_conv3x3s2_prep_bytes(cin, cout) > 0, "conv3x3s2_prepare: (cin=%d, cout=%d) unsupported", cin,
               cout);
  return split_prepare<9>("conv3x3s2_prepare", w, cin, cin, cout, prep, prep_bytes, stream);
}

// y = SiLU(conv3x3_s2((x * gc) * gp, W) + bias): x [B][cin][H][W] -> image b's output [cout][Ho][Wo] at
// y + b y_bstride (y_bstride >= cout Ho Wo: a channel slice of a concat buffer), Ho = (H + 1) / 2, Wo = (W + 1) / 2
// (Wo % 4 == 0); gc [B][cin] (16-byte aligned) and gp [B][H][W] may each be NULL (no gate).
YS_EXPORT int yolosod_conv3x3s2_silu_out(const float* x, float* y, long y_bstride, int B, int cin, int cout, int H,
                                         int W, const float* bias, const float* gc, const float* gp, const void* prep,
                                         size_t prep_bytes, void* stream) {
  YS_CHECK_ARG(x && y && bias && prep, "conv3x3s2: null pointer");
  YS_CHECK_ARG(B >= 0 && H > 0 && W > 0 && yolosod_conv3x3s2_prep_bytes(cin, cout) > 0, "conv3x3s2: bad shape");
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  YS_CHECK_ARG(Wo % 4 == 0, "conv3x3s2: output width %d not a multiple of 4", Wo);
  YS_CHECK_ARG(y_bstride >= (long)cout * Ho * Wo, "conv3x3s2: output batch stride %ld < %ld", y_bstride,
               (long)cout * Ho * Wo);
  YS_CHECK_ARG(((uintptr_t)y & 15) == 0 && y_bstride % 4 == 0, "conv3x3s2: output not 16-byte aligned");
  YS_CHECK_ARG((long)B * cin * H * W * 4 < (1L << 32) && (long)cin * H * W < (1L << 31),
               "conv3x3s2: input too large for 32-bit buffer offsets");
  YS_CHECK_ARG(!gc || ((uintptr_t)gc & 15) == 0, "conv3x3s2: channel gate must be 16-byte aligned");
  if (B == 0) return 0;
  SplitPrep sp;
  YS_CHECK_ARG(split_prep_carve(prep, prep_bytes, (size_t)2 * cout * cin * 9, &sp),
               "conv3x3s2: prepared block too small");
  const int tx = (Wo + c3s2::TW - 1) / c3s2::TW, ty = (Ho + c3s2::TH - 1) / c3s2::TH;
  const long ntiles = (long)B * tx * ty;
  YS_CHECK_ARG(ntiles < (1L << 30), "conv3x3s2: too many tiles");
  c3s2::Args a{x, sp.wp, bias, gc, gp, y, y_bstride, B, cin, H, W, Ho, Wo, tx, ty, (int)ntiles, cout / 16,
               range_flag_dev(), sp.flag};
  const int gate = (gc ? 1 : 0) | (gp ? 2 : 0);
  hipStream_t st = (hipStream_t)stream;
  using KP = void (*)(c3s2::Args);
  // persistent grids: a multiple of 8 workgroups (one per XCD slot), at most one per work item
  if (cout == 64 && cin == 32) {
    // the gated L2 conv: register-resident weights, 2-row tiles, two 256-thread workgroups per CU (4-row tiles in
    // one 512-thread workgroup measured slower)
    a.tiles_y = (Ho + 1) / 2;
    const long nt2 = (long)B * a.tiles_y * tx;
    a.ntiles = (int)nt2;
    static const KP kp[4] = {c3s2::conv3x3s2_rw_kernel<0, 2, 256>, c3s2::conv3x3s2_rw_kernel<1, 2, 256>,
                             c3s2::conv3x3s2_rw_kernel<2, 2, 256>, c3s2::conv3x3s2_rw_kernel<3, 2, 256>};
    hipLaunchKernelGGL(kp[gate], dim3((unsigned)persistent_grid(2L * cu_count(), nt2)), dim3(256), 0, st, a);
  } else {  // the tiled kernel in the form s2_form picks
    const int form = s2_form(B, cout, Ho, Wo);
    const int geo = (form & 3) - 1;
    const bool g64 = (form >> 2) == 2;
    a.tiles_x = (Wo + S2_GEO_TW[geo] - 1) / S2_GEO_TW[geo];
    a.tiles_y = (Ho + S2_GEO_TH[geo] - 1) / S2_GEO_TH[geo];
    const long nt2 = (long)B * a.tiles_y * a.tiles_x;
    const long nitems = nt2 * (g64 ? cout / 64 : cout / 128);  // work items: (tile, group)
    YS_CHECK_ARG(nitems < (1L << 30), "conv3x3s2: too many tiles");
    a.ntiles = (int)nt2;
    // workgroups per CU of the instance: three for 64-channel groups on the 32 x 2 tile, two otherwise
    const long grid = persistent_grid((g64 && geo == 0 ? 3L : 2L) * cu_count(), nitems);
#define S2T2_GATES(NCB_, G_)                                                                        \
  {                                                                                                 \
    c3s2::conv3x3s2_t2_kernel<NCB_, 0, G_>, c3s2::conv3x3s2_t2_kernel<NCB_, 1, G_>,                 \
        c3s2::conv3x3s2_t2_kernel<NCB_, 2, G_>, c3s2::conv3x3s2_t2_kernel<NCB_, 3, G_>              \
  }
    static const KP kp[3][2][4] = {{S2T2_GATES(8, 0), S2T2_GATES(4, 0)},
                                   {S2T2_GATES(8, 1), S2T2_GATES(4, 1)},
                                   {S2T2_GATES(8, 2), S2T2_GATES(4, 2)}};
#undef S2T2_GATES
    hipLaunchKernelGGL(kp[geo][g64 ? 1 : 0][gate], dim3((unsigned)grid), dim3(256), 0, st, a);
  }
  YS_CHECK_LAUNCH("conv3x3s2");
  return 0;
}

// As yolosod_conv3x3s2_silu_out with a contiguous y [B][cout][Ho][Wo].
YS_EXPORT int yolosod_conv3x3s2_silu(const float* x, float* y, int B, int cin, int cout, int H, int W,
                                     const float* bias, const float* gc, const float* gp, const void* prep,
                                     size_t prep_bytes, void* stream) {
  return yolosod_conv3x3s2_silu_out(x, y, (long)cout * ((H + 1) / 2) * ((W + 1) / 2), B, cin, cout, H, W, bias, gc, gp,
                                    prep, prep_bytes, stream);
}
