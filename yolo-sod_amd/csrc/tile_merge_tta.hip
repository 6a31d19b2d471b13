// Sliced inference with test-time augmentation, the step between the Detect head and NMS: one branch of one model call
// goes straight into the per-frame prediction tensor. y_k [n][4+nc][A_k] is the head's output for view k (scale, flip)
// of a chunk of tiles, in canvas pixels of that view; its kept anchors [src_lo, src_lo + n_k) land at anchors
// [slot*A_tot + dst_k, + n_k) of merged [F][4+nc][S*A_tot] in frame pixels. Chaining the two existing launches
// (tta.hip's tta_merge into a concatenated cat [n][4+nc][A_tot], then tile_merge.hip on cat) moves every candidate
// twice and needs cat; this is the same arithmetic in one pass, and cat is never allocated.
//
// A workgroup belongs to one destination slot (blockIdx.y = descriptor row, read with uniform loads; the descriptor is
// yolosod_tile_merge's own, unchanged), lanes run along the branch's kept anchors, every element of the branch's range
// of a named slot is written by exactly one lane (no atomics: deterministic), 4 bytes per access: A_tot is odd at the
// workload's shapes (62281 at canvas 640), so neither the slots of merged nor the branch ranges inside them start
// 16-byte aligned.
//
// Per anchor, in fp32 with IEEE division, every operation rounded on its own (the file is built with
// -ffp-contract=off; tests/tile_merge_tta_ref.py restates this in numpy):
//   step 1, tta_merge's:   x, y, w, h each / scale;  x = img_w - x (flip 3)  or  y = img_h - y (flip 2)
//   step 2, tile_merge's:  bx = (x - pad_x) / gain;  by = (y - pad_y) / gain;  bw = w / gain;  bh = h / gain
//     cut = cut_margin >= 0 and ((left interior and bx - 0.5f bw <= cut_margin) or (right interior and
//           bx + 0.5f bw >= tile_w - cut_margin) or (top ... by - 0.5f bh <= cut_margin) or (bottom ... >= tile_h - ...))
//     box = bx + off_x, by + off_y, bw, bh;  score_c = cut ? 0 : score_c
// so the result is bit for bit what the two launches give. The two divisions of a box term are not folded into one:
// x / scale / gain and x / (scale * gain) round differently.
#include "common.h"

namespace ys {

namespace tmtta {
constexpr int ROW_DW = 16;  // descriptor row: 16 dwords (64 bytes), the layout of tile_merge.hip
// dword: 0 src (row of y, -1: the slot is empty, zeros), 1 frame, 2 slot, 3 flags (bit 0 left, 1 right, 2 top,
// 3 bottom edge interior), 4 gain, 5 pad_x, 6 pad_y, 7 off_x, 8 off_y, 9 tile_w, 10 tile_h (floats), 11..15 unused
constexpr int LEFT = 1, RIGHT = 2, TOP = 4, BOTTOM = 8;
}  // namespace tmtta

__global__ __launch_bounds__(256) void tile_merge_tta_kernel(const float* __restrict__ y, int n, int nc, int A,
                                                             int src_lo, int n_k, const int* __restrict__ desc,
                                                             float* __restrict__ merged, int F, int S, int A_tot,
                                                             int dst, float scale, int flip, float img_w, float img_h,
                                                             float cut_margin) {
  using namespace tmtta;
  const int* d = desc + ROW_DW * (size_t)blockIdx.y;  // uniform loads: one slot per blockIdx.y
  const int src = d[0], frame = d[1], slot = d[2], flags = d[3];
  const float gain = __int_as_float(d[4]), pad_x = __int_as_float(d[5]), pad_y = __int_as_float(d[6]);
  const float off_x = __int_as_float(d[7]), off_y = __int_as_float(d[8]);
  const float tile_w = __int_as_float(d[9]), tile_h = __int_as_float(d[10]);
  // a row that names something outside y or merged writes nothing (the wrapper refuses such rows before the launch)
  if (src >= n || frame < 0 || frame >= F || slot < 0 || slot >= S) return;
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= n_k) return;
  const int no = 4 + nc;
  const size_t SA = (size_t)S * A_tot;
  float* out = merged + (size_t)frame * no * SA + (size_t)slot * A_tot + dst + a;
  if (src < 0) {
    for (int c = 0; c < no; ++c) out[c * SA] = 0.f;
    return;
  }
  const float* in = y + (size_t)src * no * A + src_lo + a;
  // step 1: the view's canvas pixels back to the tile's canvas
  float x = in[0] / scale, yy = in[A] / scale;
  const float w = in[2 * (size_t)A] / scale, h = in[3 * (size_t)A] / scale;
  if (flip == 3) x = img_w - x;
  if (flip == 2) yy = img_h - yy;
  // step 2: the tile's canvas back to frame pixels
  const float bx = (x - pad_x) / gain, by = (yy - pad_y) / gain, bw = w / gain, bh = h / gain;
  const float x1 = bx - 0.5f * bw, x2 = bx + 0.5f * bw, y1 = by - 0.5f * bh, y2 = by + 0.5f * bh;
  const float hi_x = tile_w - cut_margin, hi_y = tile_h - cut_margin;
  const bool cut = cut_margin >= 0.f && (((flags & LEFT) && x1 <= cut_margin) || ((flags & RIGHT) && x2 >= hi_x) ||
                                         ((flags & TOP) && y1 <= cut_margin) || ((flags & BOTTOM) && y2 >= hi_y));
  out[0] = bx + off_x;
  out[SA] = by + off_y;
  out[2 * SA] = bw;
  out[3 * SA] = bh;
  const float* sp = in + 4 * (size_t)A;
  float* op = out + 4 * SA;
  int c = 0;
  for (; c + 4 <= nc; c += 4) {  // four class rows in flight per lane
    float s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = sp[(size_t)(c + k) * A];
#pragma unroll
    for (int k = 0; k < 4; ++k) op[(c + k) * SA] = cut ? 0.f : s[k];
  }
#pragma clang loop vectorize(disable)
  for (; c < nc; ++c) op[c * SA] = cut ? 0.f : sp[(size_t)c * A];
}

}  // namespace ys

using namespace ys;

YS_EXPORT int yolosod_tile_merge_tta(const float* y, int n, int nc, int A, int src_lo, int n_k, const int32_t* desc,
                                     int rows, float* merged, int F, int S, int A_tot, int dst, float scale, int flip,
                                     float img_w, float img_h, float cut_margin, void* stream) {
  YS_CHECK_ARG(y && desc && merged, "tile_merge_tta: null pointer");
  YS_CHECK_ARG(n >= 1, "tile_merge_tta: n=%d", n);
  YS_CHECK_ARG(nc >= 1 && nc <= 64, "tile_merge_tta: nc=%d unsupported (1..64)", nc);
  YS_CHECK_ARG(A >= 1 && A_tot >= 1, "tile_merge_tta: A=%d, A_tot=%d", A, A_tot);
  YS_CHECK_ARG(S >= 1 && F >= 1, "tile_merge_tta: F=%d, S=%d", F, S);
  YS_CHECK_ARG((double)S * (double)A_tot * (double)nc < 4294967296.0, "tile_merge_tta: S*A_tot*nc = %d*%d*%d >= 2^32",
               S, A_tot, nc);
  YS_CHECK_ARG((double)A * (4 + nc) < 2147483648.0, "tile_merge_tta: A * (4 + nc) >= 2^31");
  YS_CHECK_ARG(rows >= 1 && rows <= 65535, "tile_merge_tta: rows=%d unsupported (1..65535)", rows);
  YS_CHECK_ARG(n_k >= 1 && src_lo >= 0 && (long)src_lo + n_k <= A,
               "tile_merge_tta: source anchors [%d, %d + %d) leave y's %d", src_lo, src_lo, n_k, A);
  YS_CHECK_ARG(dst >= 0 && (long)dst + n_k <= A_tot, "tile_merge_tta: destination anchors [%d, %d + %d) leave a slot's %d",
               dst, dst, n_k, A_tot);
  YS_CHECK_ARG(scale > 0.f && scale < __builtin_inff(), "tile_merge_tta: scale must be finite and > 0");
  YS_CHECK_ARG(flip == 0 || flip == 2 || flip == 3, "tile_merge_tta: flip=%d (0, 2 or 3)", flip);
  YS_CHECK_ARG(!(img_w != img_w) && !(img_h != img_h), "tile_merge_tta: image size is NaN");
  YS_CHECK_ARG(!(cut_margin != cut_margin), "tile_merge_tta: cut_margin is NaN");
  YS_CHECK_ARG(((uintptr_t)desc & 3) == 0 && ((uintptr_t)y & 3) == 0 && ((uintptr_t)merged & 3) == 0,
               "tile_merge_tta: misaligned pointer");
  const dim3 grid((unsigned)((n_k + 255) / 256), (unsigned)rows);
  hipLaunchKernelGGL(tile_merge_tta_kernel, grid, dim3(256), 0, (hipStream_t)stream, y, n, nc, A, src_lo, n_k,
                     (const int*)desc, merged, F, S, A_tot, dst, scale, flip, img_w, img_h, cut_margin);
  YS_CHECK_LAUNCH("tile_merge_tta");
  return 0;
}
