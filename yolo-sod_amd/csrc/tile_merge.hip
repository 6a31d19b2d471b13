// Sliced inference, the step between the Detect head and NMS: the head's output for a chunk of tiles, y [n][4+nc][A]
// (xywh in canvas pixels + sigmoid scores, each tile letterboxed onto the common canvas), becomes one prediction
// tensor per frame, merged [F][4+nc][S*A] in frame pixels, slot s of a frame at anchors [s*A, (s+1)*A). One NMS over
// merged[f] then de-duplicates the candidates of every tile (and of the whole-frame slot) of frame f at once.
//
// Written with torch ops this is, per tile, a slice, four arithmetic passes over the box rows, a mask pass and a
// strided copy. Here it is one pass: a workgroup belongs to one destination slot (blockIdx.y = descriptor row, read
// with uniform loads), lanes run along the anchors, every element of a named slot is written by exactly one lane (no
// atomics: deterministic), 16 bytes per access when A % 4 == 0 (then every row of y and every slot of merged starts
// 16-byte aligned) and element by element for any other A.
//
// Per anchor, in fp32 with IEEE division (the way back is scale_boxes' (v - pad) / gain, then the tile's offset):
//   bx = (x - pad_x) / gain;  by = (y - pad_y) / gain;  bw = w / gain;  bh = h / gain
//   cut = cut_margin >= 0 and ((left interior and bx - 0.5f bw <= cut_margin) or (right interior and
//         bx + 0.5f bw >= tile_w - cut_margin) or (top ...  by - 0.5f bh <= cut_margin) or (bottom ... >= tile_h - ...))
//   box = bx + off_x, by + off_y, bw, bh;  score_c = cut ? 0 : score_c
// A box that a tile border truncates is seen whole by a neighbouring tile or by the whole-frame slot; `cut` removes the
// truncated copy before NMS. Multiplying by 0.5f is exact (barring underflow to a subnormal), so bx -+ 0.5f bw rounds
// once whether or not the compiler contracts it into an FMA: the result does not depend on -ffp-contract (the file
// is built with it off all the same, as nms.hip and detect.hip are; tests/tile_merge_ref.py restates this in numpy).
#include <type_traits>

#include "common.h"

namespace ys {

namespace tmerge {
constexpr int ROW_DW = 16;  // descriptor row: 16 dwords (64 bytes)
// dword: 0 src (row of y, -1: the slot is empty, zeros), 1 frame, 2 slot, 3 flags (bit 0 left, 1 right, 2 top,
// 3 bottom edge interior), 4 gain, 5 pad_x, 6 pad_y, 7 off_x, 8 off_y, 9 tile_w, 10 tile_h (floats), 11..15 unused
constexpr int LEFT = 1, RIGHT = 2, TOP = 4, BOTTOM = 8;
}  // namespace tmerge

template <class V>
__device__ __forceinline__ V splat(float v);
template <>
__device__ __forceinline__ float splat<float>(float v) { return v; }
template <>
__device__ __forceinline__ f32x4 splat<f32x4>(float v) { return f32x4{v, v, v, v}; }

__device__ __forceinline__ float sel(bool c, float a, float b) { return c ? a : b; }
__device__ __forceinline__ f32x4 sel(const bool* c, f32x4 a, f32x4 b) {
  return f32x4{c[0] ? a.x : b.x, c[1] ? a.y : b.y, c[2] ? a.z : b.z, c[3] ? a.w : b.w};
}

// VEC anchors per lane (4: 16-byte accesses, A % 4 == 0; 1: any A)
template <int VEC>
__global__ __launch_bounds__(256) void tile_merge_kernel(const float* __restrict__ y, int n, int nc, int A,
                                                         const int* __restrict__ desc, float* __restrict__ merged,
                                                         int F, int S, float cut_margin) {
  using namespace tmerge;
  using V = typename std::conditional<VEC == 4, f32x4, float>::type;
  const int* d = desc + ROW_DW * (size_t)blockIdx.y;  // uniform loads: one slot per blockIdx.y
  const int src = d[0], frame = d[1], slot = d[2], flags = d[3];
  const float gain = __int_as_float(d[4]), pad_x = __int_as_float(d[5]), pad_y = __int_as_float(d[6]);
  const float off_x = __int_as_float(d[7]), off_y = __int_as_float(d[8]);
  const float tile_w = __int_as_float(d[9]), tile_h = __int_as_float(d[10]);
  // a row that names something outside y or merged writes nothing (the wrapper refuses such rows before the launch)
  if (src >= n || frame < 0 || frame >= F || slot < 0 || slot >= S) return;
  const long a = ((long)blockIdx.x * 256 + threadIdx.x) * VEC;
  if (a >= A) return;  // VEC == 4: A % 4 == 0, so a lane's four anchors are inside or outside together
  const int no = 4 + nc;
  const size_t SA = (size_t)S * A;
  float* out = merged + (size_t)frame * no * SA + (size_t)slot * A + a;
  if (src < 0) {
    for (int c = 0; c < no; ++c) *reinterpret_cast<V*>(out + c * SA) = splat<V>(0.f);
    return;
  }
  const float* in = y + (size_t)src * no * A + a;
  const V x = *reinterpret_cast<const V*>(in), yy = *reinterpret_cast<const V*>(in + A);
  const V w = *reinterpret_cast<const V*>(in + 2 * (size_t)A), h = *reinterpret_cast<const V*>(in + 3 * (size_t)A);
  const V bx = (x - pad_x) / gain, by = (yy - pad_y) / gain, bw = w / gain, bh = h / gain;
  const V x1 = bx - 0.5f * bw, x2 = bx + 0.5f * bw, y1 = by - 0.5f * bh, y2 = by + 0.5f * bh;
  const float hi_x = tile_w - cut_margin, hi_y = tile_h - cut_margin;
  const bool on = cut_margin >= 0.f;
  bool cut[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    float x1j, x2j, y1j, y2j;
    if constexpr (VEC == 4) {
      x1j = x1[j], x2j = x2[j], y1j = y1[j], y2j = y2[j];
    } else {
      x1j = x1, x2j = x2, y1j = y1, y2j = y2;
    }
    cut[j] = on && (((flags & LEFT) && x1j <= cut_margin) || ((flags & RIGHT) && x2j >= hi_x) ||
                    ((flags & TOP) && y1j <= cut_margin) || ((flags & BOTTOM) && y2j >= hi_y));
  }
  *reinterpret_cast<V*>(out) = bx + off_x;
  *reinterpret_cast<V*>(out + SA) = by + off_y;
  *reinterpret_cast<V*>(out + 2 * SA) = bw;
  *reinterpret_cast<V*>(out + 3 * SA) = bh;
  const float* sp = in + 4 * (size_t)A;
  float* op = out + 4 * SA;
  int c = 0;
  for (; c + 4 <= nc; c += 4) {  // four class rows in flight per lane
    V s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = *reinterpret_cast<const V*>(sp + (size_t)(c + k) * A);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if constexpr (VEC == 4) *reinterpret_cast<V*>(op + (c + k) * SA) = sel(cut, splat<V>(0.f), s[k]);
      else *reinterpret_cast<V*>(op + (c + k) * SA) = sel(cut[0], 0.f, s[k]);
    }
  }
  for (; c < nc; ++c) {
    const V s = *reinterpret_cast<const V*>(sp + (size_t)c * A);
    if constexpr (VEC == 4) *reinterpret_cast<V*>(op + c * SA) = sel(cut, splat<V>(0.f), s);
    else *reinterpret_cast<V*>(op + c * SA) = sel(cut[0], 0.f, s);
  }
}

}  // namespace ys

using namespace ys;

YS_EXPORT int yolosod_tile_merge(const float* y, int n, int nc, int A, const int32_t* desc, int rows, float* merged,
                                 int F, int S, float cut_margin, void* stream) {
  YS_CHECK_ARG(y && desc && merged, "tile_merge: null pointer");
  YS_CHECK_ARG(n >= 1, "tile_merge: n=%d", n);
  YS_CHECK_ARG(nc >= 1 && nc <= 64, "tile_merge: nc=%d unsupported (1..64)", nc);
  YS_CHECK_ARG(A >= 1, "tile_merge: A=%d", A);
  YS_CHECK_ARG(S >= 1 && F >= 1, "tile_merge: F=%d, S=%d", F, S);
  YS_CHECK_ARG((double)S * (double)A * (double)nc < 4294967296.0, "tile_merge: S*A*nc = %d*%d*%d >= 2^32", S, A, nc);
  YS_CHECK_ARG(rows >= 1 && rows <= 65535, "tile_merge: rows=%d unsupported (1..65535)", rows);
  YS_CHECK_ARG(((uintptr_t)desc & 3) == 0 && ((uintptr_t)y & 3) == 0 && ((uintptr_t)merged & 3) == 0,
               "tile_merge: misaligned pointer");
  YS_CHECK_ARG(!(cut_margin != cut_margin), "tile_merge: cut_margin is NaN");
  hipStream_t st = (hipStream_t)stream;
  const bool vec = A % 4 == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)merged & 15) == 0;
  if (vec) {
    const dim3 grid((unsigned)((A / 4 + 255) / 256), (unsigned)rows);
    hipLaunchKernelGGL(tile_merge_kernel<4>, grid, dim3(256), 0, st, y, n, nc, A, (const int*)desc, merged, F, S,
                       cut_margin);
  } else {
    const dim3 grid((unsigned)((A + 255) / 256), (unsigned)rows);
    hipLaunchKernelGGL(tile_merge_kernel<1>, grid, dim3(256), 0, st, y, n, nc, A, (const int*)desc, merged, F, S,
                       cut_margin);
  }
  YS_CHECK_LAUNCH("tile_merge");
  return 0;
}
