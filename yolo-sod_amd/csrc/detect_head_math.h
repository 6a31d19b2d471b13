// The arithmetic of the Detect head's fp16-split tail (detect.hip: detect_head_x2_kernel) as one text, shared with the
// tower conv that runs the same tail in its epilogue (conv3x3.hip: conv3x3_head_kernel), so that the two give the same
// bits: the 1x1 conv of one 16-pixel group on v_mfma_f32_16x16x32_f16 with the weights as the A operand, the DFL
// expectation, dist2bbox and the class sigmoid.
//
// Weight planes [t][s][g][row][i] of 64 W (hi plane, lo plane): 16-row output tile t, k step s (32 channels), lane
// group g, row of the tile, k slot i: W[16 t + row][g + 32 s + 4 i], that is, lane (g, j)'s A fragment of (t, s) is the
// 8 halves at ((t NS + s) 64 + 16 g + j) 8. The features are the B operand: lane (g, j) holds channels g + 4 q of
// pixel j, q = 8 s + i.
//
// Every function body is compiled with fp contraction off, whatever the including file's setting: the head's decode
// must round like the reference's fp32 code (detect.hip is built with -ffp-contract=off as a whole).
#pragma once
#include "common.h"

namespace ys {
namespace headm {

constexpr float WS = 64.0f;  // weight scale (exact)

// One thread per pair of neighbouring k slots: element pair e of the planes of W [rows][64] (rows past `rows` zero)
// -> the pair's scaled values, as the head kernel builds them per workgroup.
__device__ __forceinline__ f32x2 weight_pair(const float* w, int rows, int e) {
#pragma clang fp contract(off)
  const int i = e & 7, row = (e >> 3) & 15, gg = (e >> 7) & 3, s = (e >> 9) & 1, t = e >> 10;
  const int r = 16 * t + row;
  const float* src = w + (r < rows ? r : 0) * 64 + gg + 32 * s + 4 * i;
  return r < rows ? f32x2{src[0], src[4]} * WS : f32x2{0.f, 0.f};
}

// acc[t] += W(t, .) . c for NT output tiles over NSTEP k steps: c[8 s + i] is the lane's feature of k slot i in step
// s; wf(idx, plane) returns the lane's A fragment of (tile, step) idx = t NSTEP + s (plane 0 hi, 1 lo). The split of
// the features and the split-range maximum are the head kernel's.
template <int NT, int NSTEP, class WF>
__device__ __forceinline__ void mma(const float (&c)[8 * NSTEP], WF&& wf, f32x4 (&acc)[NT], float& rng) {
#pragma unroll
  for (int s = 0; s < NSTEP; ++s) {
    f16x8_t fh, fl;
    const f32x4 va{c[8 * s], c[8 * s + 1], c[8 * s + 2], c[8 * s + 3]};
    const f32x4 vb{c[8 * s + 4], c[8 * s + 5], c[8 * s + 6], c[8 * s + 7]};
    split8x(va, vb, fh, fl);  // features that come from memory: the 3-VALU split (common.h split2x)
    rng = range_acc(range_acc(rng, va), vb);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = mfma_f16x3(wf(t * NSTEP + s, 0), wf(t * NSTEP + s, 1), fh, fl, acc[t]);
  }
}

// DFL (block.py:79-82) of the four box tiles: lane (g, j) holds bins 4 g .. + 3 of side s of pixel j in acc[s];
// bb[s][r]: the bias of bin 4 g + r of side s. Every lane of the wave takes part (permlane swaps).
__device__ __forceinline__ void dfl(const f32x4 (&acc)[4], const float (&bb)[4][4], int g, float (&dist)[4]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = acc[s][r] * (1.0f / WS) + bb[s][r];
    float mx = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
    mx = xor32_max(xor16_max(mx));
    float sum = 0.f, e = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      v[r] = __expf(v[r] - mx);
      sum += v[r];
      e += (float)(4 * g + r) * v[r];
    }
    sum = xor32_sum(xor16_sum(sum));
    e = xor32_sum(xor16_sum(e));
    dist[s] = e * __builtin_amdgcn_rcpf(sum);
  }
}

// dist2bbox (utils/tal.py:345-357, xywh) of the anchor at column ix, row iy, times the level's stride: lane group g's
// output row (0 cx, 1 cy, 2 w, 3 h).
__device__ __forceinline__ float box_out(const float (&dist)[4], int ix, int iy, float st, int g) {
#pragma clang fp contract(off)
  const float ax = (float)ix + 0.5f, ay = (float)iy + 0.5f;
  const float x1 = ax - dist[0], y1 = ay - dist[1];
  const float x2 = ax + dist[2], y2 = ay + dist[3];
  return g == 0 ? ((x1 + x2) / 2.0f) * st : g == 1 ? ((y1 + y2) / 2.0f) * st : g == 2 ? (x2 - x1) * st : (y2 - y1) * st;
}

// class score: sigmoid on the hardware exp2 / rcp (1-2 ulp; the libm expf + IEEE division were ~15 % of the head
// kernel's VALU, and the split products already carry a few ulp)
__device__ __forceinline__ float cls_out(float acc, float bias) {
#pragma clang fp contract(off)
  return sigmoid_fast_(acc * (1.0f / WS) + bias);
}

}  // namespace headm
}  // namespace ys
