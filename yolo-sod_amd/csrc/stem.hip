// The stem: out = SiLU(conv3x3 / stride 2 / pad 1 (x, w) + bias) for fp32 NCHW with Cin = 3 (layer 0 of the YAMLs,
// 3 -> 32 at 640^2 -> 320^2), plus the per-plane partial sums the following SE reads, in one pass over the image.
//
// MIOpen ran this layer as a Winograd kernel followed by the bias / SiLU / statistics epilogue: the 32-channel
// full-resolution map was written, read and written again. Here a workgroup stages the 17 x 129 input window of an
// 8 x 64 output tile (all three channels) in LDS once, every lane keeps the 3 x 3 x 9 inputs of four consecutive
// output pixels in registers and walks the output channels with the 27 weights of each in scalar registers (uniform
// loads of the fused Conv's own weight tensor: no prepared block). K = 27 is far too thin for the matrix cores, and
// plain fp32 FMAs in a fixed (ci, ky, kx) order keep the layer exact: the only difference from the MIOpen path is the
// summation order of the 27 products. Each output plane is written with 16-byte stores (a row of 16 lanes = 256
// contiguous bytes).
//
// Statistics: a lane's four stored values are summed, the workgroup reduces them per output channel in a fixed order
// into two slots per tile - the part of the tile in the plan segment of its first pixel, and the part in the next one
// (a segment boundary may fall inside a row; 16-byte groups never straddle one since seg % 4 == 0) - and a second,
// tiny kernel adds the tiles of every (plane, segment) in tile order. No atomics: the result is deterministic.
#include "common.h"
#include <math.h>

namespace ys {

namespace stem {
constexpr int TR = 8;              // output rows per tile
constexpr int TW = 64;             // output columns per tile
constexpr int LR = 2 * TR + 1;     // staged input rows per channel
constexpr int LS = 2 * TW + 8;     // LDS row stride: [3] = left halo, [4, 4 + 2 TW) = the tile's columns
constexpr int SLOTS = 2 * TW / 4 + 1;  // staging work items per row: the halo + 32 float4
constexpr int QUADS = TR * TW / 4;     // 128 four-pixel groups per tile
constexpr int MAXC = 64;
constexpr int LDS_FLOATS = (3 * LR * LS > MAXC * QUADS) ? 3 * LR * LS : MAXC * QUADS;
}  // namespace stem

__global__ __launch_bounds__(256) void stem_conv_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ out,
                                                        int Cout, int H, int W, int Ho, int Wo, int ntx, int nty,
                                                        long seg, float* __restrict__ tws) {
  using namespace stem;
  __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
  const int tid = threadIdx.x;
  const int bx = blockIdx.x;
  const int tx = bx % ntx;
  const int ty = (bx / ntx) % nty;
  const int b = bx / (ntx * nty);
  const int r0 = ty * TR, c0 = tx * TW;
  const float* xb = x + (size_t)b * 3 * H * W;

  // ---- stage input rows [2 r0 - 1, 2 r0 + 2 TR) x columns [2 c0 - 1, 2 c0 + 2 TW) of the three channels; zeros outside
  // Item (row, s): the 16-byte group at columns 2 c0 - 4 + 4 s (s = 0 holds the left halo in its last element). Every
  // item is one unconditional load from an address clamped into the image (W % 4 == 0: a group is inside or outside as
  // a whole), zeroed afterwards when outside: all of a thread's loads are in flight before the first LDS store.
  const int ir0 = 2 * r0 - 1, ic0 = 2 * c0;
  constexpr int NSTG = (3 * LR * SLOTS + 255) / 256;
  f32x4 sv[NSTG];
#pragma unroll
  for (int it = 0; it < NSTG; ++it) {
    const int i = min(it * 256 + tid, 3 * LR * SLOTS - 1);
    const int row = i / SLOTS;  // ci * LR + lr
    const int s = i - row * SLOTS;
    const int ci = row / LR;
    const int gr = ir0 + (row - ci * LR), gc = ic0 - 4 + 4 * s;
    const bool ok = gr >= 0 && gr < H && gc >= 0 && gc < W;
    sv[it] = ld4(xb + ((size_t)ci * H + (ok ? gr : 0)) * W + (ok ? gc : 0));
    if (!ok) sv[it] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int it = 0; it < NSTG; ++it) {
    const int i = it * 256 + tid;
    if (i < 3 * LR * SLOTS) st4(&lds[(i / SLOTS) * LS + 4 * (i % SLOTS)], sv[it]);
  }
  __syncthreads();

  // ---- this lane's four output pixels: row r0 + ry, columns c0 + 4 xq .. + 3; the 3 x 3 x 9 inputs they read
  const int q = tid & (QUADS - 1);
  const int ry = q >> 4, xq = q & 15;
  const int half = __builtin_amdgcn_readfirstlane(tid >> 7);  // waves 0, 1: the first Cout / 2 channels
  float in[3][3][9];
#pragma unroll
  for (int ci = 0; ci < 3; ++ci)
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const float* lr = &lds[(ci * LR + 2 * ry + ky) * LS + 8 * xq];
      in[ci][ky][0] = lr[3];
      const f32x4 a = ld4(lr + 4), c = ld4(lr + 8);
      in[ci][ky][1] = a.x; in[ci][ky][2] = a.y; in[ci][ky][3] = a.z; in[ci][ky][4] = a.w;
      in[ci][ky][5] = c.x; in[ci][ky][6] = c.y; in[ci][ky][7] = c.z; in[ci][ky][8] = c.w;
    }
  __syncthreads();  // the staged tile is in registers: the LDS block becomes the statistics scratch

  const int orow = r0 + ry, ocol = c0 + 4 * xq;
  const bool valid = orow < Ho && ocol < Wo;  // Wo % 4 == 0
  const int nh = Cout >> 1;
  for (int cc = 0; cc < nh; ++cc) {
    const int co = half * nh + cc;
    const float* wc = w + co * 27;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ci = 0; ci < 3; ++ci)
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const float wv = wc[ci * 9 + ky * 3 + kx];
          acc.x = __builtin_fmaf(in[ci][ky][kx], wv, acc.x);
          acc.y = __builtin_fmaf(in[ci][ky][kx + 2], wv, acc.y);
          acc.z = __builtin_fmaf(in[ci][ky][kx + 4], wv, acc.z);
          acc.w = __builtin_fmaf(in[ci][ky][kx + 6], wv, acc.w);
        }
    acc += bias[co];
    f32x4 o = {silu_st<float>(acc.x), silu_st<float>(acc.y), silu_st<float>(acc.z), silu_st<float>(acc.w)};
    float s = 0.f;
    if (valid) {
      st4(out + (((size_t)b * Cout + co) * Ho + orow) * Wo + ocol, o);
      s = (o.x + o.y) + (o.z + o.w);  // statistics of the stored values
    }
    lds[co * QUADS + q] = s;
  }
  __syncthreads();

  // ---- per channel: tile row p by lane p of an 8-lane group (16 groups in row order), then the 8 rows; slot 0 = the
  // segment of the tile's first pixel, slot 1 = the next one
  const long first = (long)r0 * Wo + c0;
  const long bound = (first / seg + 1) * seg;
  const int p = tid & 7;
  for (int co = tid >> 3; co < Cout; co += 32) {
    const long base = (long)(r0 + p) * Wo + c0;
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float v = lds[co * QUADS + p * 16 + j];
      const bool hi = base + 4 * j >= bound;
      a0 += hi ? 0.f : v;
      a1 += hi ? v : 0.f;
    }
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) {
      a0 += __shfl_xor(a0, m, 64);
      a1 += __shfl_xor(a1, m, 64);
    }
    if (p == 0) {
      float* t = tws + ((((size_t)b * Cout + co) * nty + ty) * ntx + tx) * 2;
      t[0] = a0;
      t[1] = a1;
    }
  }
}

// psum[plane * parts + k] = the tiles' contributions to segment k, in tile order
__global__ __launch_bounds__(256) void stem_stats_reduce_kernel(const float* __restrict__ tws,
                                                                float* __restrict__ psum, long total, int parts,
                                                                long seg, long HW, int Wo, int ntx, int nty) {
  using namespace stem;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long plane = i / parts;
  const int k = (int)(i - plane * parts);
  const long s0 = k * seg;
  const long s1 = (s0 + seg < HW) ? s0 + seg : HW;
  const int ty0 = (int)(s0 / Wo) / TR, ty1 = (int)((s1 - 1) / Wo) / TR;
  float s = 0.f;
  for (int ty = ty0; ty <= ty1; ++ty)
    for (int tx = 0; tx < ntx; ++tx) {
      const int k0 = (ty * TR * Wo + tx * TW) / (int)seg;  // HW < 2^31 (host check)
      const float* t = tws + ((plane * nty + ty) * ntx + tx) * 2;
      if (k0 == k) s += t[0];
      else if (k0 + 1 == k) s += t[1];
    }
  psum[i] = s;
}

}  // namespace ys

using namespace ys;

// floats of tile scratch yolosod_stem_conv needs
YS_EXPORT size_t yolosod_stem_workspace(int B, int Cout, int H, int W) {
  if (B <= 0 || Cout <= 0 || H <= 0 || W <= 0) return 0;
  const int Ho = H / 2, Wo = W / 2;
  const size_t nty = (Ho + stem::TR - 1) / stem::TR, ntx = (Wo + stem::TW - 1) / stem::TW;
  return sizeof(float) * 2 * (size_t)B * Cout * nty * ntx;
}

// out [B, Cout, H/2, W/2] = SiLU(conv3x3 s2 p1 (x [B, 3, H, W], w [Cout, 3, 3, 3]) + bias), contiguous fp32, and
// psum [B * Cout * parts] in the segmentation yolosod_plane_parts(H/2 * W/2) gives (parts, seg). H, W even,
// (W/2) % 4 == 0, Cout even and <= 64, 16-byte aligned x / out.
YS_EXPORT int yolosod_stem_conv(const float* x, const float* w, const float* bias, float* out, int B, int Cout, int H,
                                int W, int parts, long seg, float* psum, void* workspace, size_t workspace_bytes,
                                void* stream) {
  using namespace stem;
  YS_CHECK_ARG(x && w && bias && out && psum, "stem_conv: null pointer");
  YS_CHECK_ARG(B >= 0 && H > 0 && W > 0 && H % 2 == 0 && W % 8 == 0, "stem_conv: H even and W %% 8 == 0 required");
  YS_CHECK_ARG(Cout > 0 && Cout % 2 == 0 && Cout <= MAXC, "stem_conv: Cout=%d unsupported (even, <= %d)", Cout, MAXC);
  YS_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0, "stem_conv: x / out must be 16-byte aligned");
  const int Ho = H / 2, Wo = W / 2;
  const long HW = (long)Ho * Wo;
  YS_CHECK_ARG(HW < (1L << 31), "stem_conv: plane of %ld pixels too large", HW);
  YS_CHECK_ARG(parts >= 1 && seg > 0 && seg % 4 == 0 && (long)parts * seg >= HW && (long)(parts - 1) * seg < HW,
               "stem_conv: plane plan (%d x %ld) does not cover HW=%ld", parts, seg, HW);
  // a tile (8 output rows) meets at most two segments
  YS_CHECK_ARG(parts == 1 || (long)TR * Wo <= seg, "stem_conv: segment of %ld shorter than %d rows of %d", seg, TR, Wo);
  if (B == 0) return 0;
  const int nty = (Ho + TR - 1) / TR, ntx = (Wo + TW - 1) / TW;
  const long blocks = (long)B * nty * ntx;
  YS_CHECK_ARG(blocks < (1L << 31) && (size_t)B * 3 * H * W < ((size_t)1 << 40), "stem_conv: too many tiles");
  YS_CHECK_ARG(workspace && workspace_bytes >= yolosod_stem_workspace(B, Cout, H, W),
               "stem_conv: workspace too small (%zu)", workspace_bytes);
  hipStream_t st = (hipStream_t)stream;
  float* tws = (float*)workspace;
  hipLaunchKernelGGL(stem_conv_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, w, bias, out, Cout, H, W, Ho, Wo,
                     ntx, nty, seg, tws);
  YS_CHECK_LAUNCH("stem_conv");
  const long total = (long)B * Cout * parts;
  hipLaunchKernelGGL(stem_stats_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                     (const float*)tws, psum, total, parts, seg, HW, Wo, ntx, nty);
  YS_CHECK_LAUNCH("stem_stats_reduce");
  return 0;
}
