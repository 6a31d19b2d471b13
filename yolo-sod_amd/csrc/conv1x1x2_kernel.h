// The kernel of csrc/conv1x1x2.hip, included there twice inside ys::c1 (no include guard): once as it always was
// (conv1x1_x2_kernel<DUAL, NP, CPW, DB>) and once, with YS_C1_STATS_FORMS defined, as the statistics forms
// (conv1x1_x2s_kernel<CPW, STATS>). One text for both, so that the first family's instances compile to the code they
// had before the statistics forms existed, under the names they had.

// NP pixels per tile (64 or 128: the weights are read from L2 once per tile, 128 halves that traffic)
// CPW: 16-channel output blocks per wave (2: workgroups of 128 output channels; 4: of 256; 1: of 64, for Cout 64)
// DB: the staged planes are double-buffered (one barrier per stage)
// STATS: 0, or the epilogue also writes the tile's per-channel sum (1) / sum and max (2) of the stored values
#ifdef YS_C1_STATS_FORMS
// the statistics forms: 64-pixel tiles, one store, one pair of staged planes; kernels of their own name
template <int CPW, int STATS>
__global__ __launch_bounds__(NT, 2) void conv1x1_x2s_kernel(Args p) {
  constexpr bool DUAL = false, DB = false;
  constexpr int NP = 64;
  static_assert(STATS == 1 || STATS == 2, "STATS");
#else
template <bool DUAL, int NP, int CPW = 2, bool DB = false>
__global__ __launch_bounds__(NT, 2) void conv1x1_x2_kernel(Args p) {
  constexpr int STATS = 0;
#endif
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
    float ts = 0.f, tm = -INFINITY;
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
        if (STATS) {  // pixels past HW were staged as copies of the last pixel: not counted
          ts += (v[0] + v[1]) + (v[2] + v[3]);
          if (STATS == 2) tm = nmax_(tm, nmax4_(v[0], v[1], v[2], v[3]));  // NaN-propagating (common.h nmax_)
        }
      }
    }
    if (STATS) {  // the four lane groups of a channel hold its 64 pixels
      ts += __shfl_xor(ts, 16, 64);
      ts += __shfl_xor(ts, 32, 64);
      if (STATS == 2) {
        tm = nmax_(tm, __shfl_xor(tm, 16, 64));
        tm = nmax_(tm, __shfl_xor(tm, 32, 64));
      }
      if (g == 0) {
        const long ti = ((long)b * p.cout + o) * p.ntile + tile;
        p.y2[ti] = ts;
        if (STATS == 2) p.y2[p.y2bs + ti] = tm;
      }
    }
  }
  range_report(p.range_flag, rng);
  if (p.prep_flag && p.range_flag && blockIdx.x == 0 && threadIdx.x == 0 && *p.prep_flag) *p.range_flag = 1u;
}
