// Test-time augmentation around the model calls (ultralytics/nn/tasks.py:381-418 _predict_augment): the scaled /
// flipped views of a batch in ONE launch (scale_img, utils/torch_utils.py:423-432, after x.flip), and per model call one
// launch that de-scales, de-flips, clips the tail and places that branch's anchors in the concatenated prediction
// tensor (_descale_pred + _clip_augmented + torch.cat).
//
// Written with torch ops the views are flip + F.interpolate + F.pad per view (three full passes each) and the merge an
// in-place divide, a split, a subtract and two cats per branch. Here every output element of a view is written exactly
// once by one lane (four pixels per lane, one 16-byte / 8-byte store), and every element of a branch's range of the
// concatenated tensor exactly once (lanes along the anchors, 4-byte accesses: A_tot is odd at the workload's own shape,
// so the rows of cat cannot be 16-byte aligned). No atomics: deterministic.
//
// Both are specified bit for bit (tests/tta_ref.py restates them in numpy float32); the file is built with
// -ffp-contract=off so that every product and sum below rounds on its own.
// Resize, per axis, n_in -> n_out, destination index d (aten's bilinear, align_corners=False, no antialias):
//   scale = float(n_in) / float(n_out);  src = max(scale * (d + 0.5f) - 0.5f, 0)
//   i0 = min((int)src, n_in - 1);  i1 = i0 + (i0 < n_in - 1);  l1 = src - i0;  l0 = 1 - l1
//   a flip of the axis replaces index i by n_in - 1 - i
//   value = ly0 * (lx0 * p[y0][x0] + lx1 * p[y0][x1]) + ly1 * (lx0 * p[y1][x0] + lx1 * p[y1][x1])
// bf16 input is widened first and the fp32 value rounded once to nearest even; the pad is 0.447f (bf16: its rounding).
// Merge, per anchor: x, y, w, h each / float32(scale) (IEEE division), then x = float32(img_w) - x (flip 3) or
// y = float32(img_h) - y (flip 2); the scores are copied.
#include "common.h"

namespace ys {

namespace tta {
constexpr int TH = 16;         // output rows per workgroup
constexpr int TW = 64;         // output columns per workgroup (16 lanes x 4 pixels)
constexpr int MAXDIM = 16384;  // extents (indices and d + 0.5f exact in fp32 by a wide margin)
constexpr float PAD = 0.447f;  // scale_img's border (the ImageNet mean)
}  // namespace tta

typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));

struct TtaAxis {
  int i0, i1;
  float l0, l1;
};

__device__ __forceinline__ TtaAxis tta_axis(int d, int n_in, float scale, bool flip) {
  float src = scale * ((float)d + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  int i0 = (int)src;
  i0 = i0 < n_in - 1 ? i0 : n_in - 1;
  int i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  const float l1 = src - (float)i0;
  const float l0 = 1.0f - l1;
  if (flip) {
    i0 = n_in - 1 - i0;
    i1 = n_in - 1 - i1;
  }
  return TtaAxis{i0, i1, l0, l1};
}

// desc [V][8] int64: output address, flip (0 none, 2 up-down, 3 left-right), sh, sw (resized), ph, pw (padded), 0, 0
// grid: x = column tiles of the widest view, y = row tiles of the tallest, z = view * planes + plane (plane = b * C + c)
template <class T>
__global__ __launch_bounds__(256) void tta_views_kernel(const T* __restrict__ x, int planes, int H, int W,
                                                        const int64_t* __restrict__ desc, int V, int max_ph,
                                                        int max_pw) {
  using namespace tta;
  const int v = blockIdx.z / planes, plane = blockIdx.z - v * planes;
  const int64_t* d = desc + 8 * (size_t)v;  // uniform loads: one view per blockIdx.z / planes
  T* out = (T*)(uintptr_t)d[0];
  const int flip = (int)d[1], sh = (int)d[2], sw = (int)d[3], ph = (int)d[4], pw = (int)d[5];
  // a row that names sizes the launch was not sized for writes nothing (the wrapper refuses such rows before)
  if (v >= V || ph < 1 || pw < 4 || (pw & 3) || ph > max_ph || pw > max_pw || sh < 1 || sw < 1 || sh > ph || sw > pw)
    return;
  const int row = blockIdx.y * TH + (threadIdx.x >> 4), col = blockIdx.x * TW + 4 * (threadIdx.x & 15);
  if (row >= ph || col >= pw) return;  // pw % 4 == 0: a lane's four pixels are inside or outside together
  f32x4 o = {PAD, PAD, PAD, PAD};
  if (row < sh && col < sw) {
    const float sy = (float)H / (float)sh, sx = (float)W / (float)sw;
    const TtaAxis ay = tta_axis(row, H, sy, flip == 2);
    const T* p0 = x + (size_t)plane * H * W + (size_t)ay.i0 * W;
    const T* p1 = x + (size_t)plane * H * W + (size_t)ay.i1 * W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (col + j < sw) {
        const TtaAxis ax = tta_axis(col + j, W, sx, flip == 3);
        const float a = ld1(p0 + ax.i0), b = ld1(p0 + ax.i1), c = ld1(p1 + ax.i0), e = ld1(p1 + ax.i1);
        o[j] = ay.l0 * (ax.l0 * a + ax.l1 * b) + ay.l1 * (ax.l0 * c + ax.l1 * e);
      }
    }
  }
  // the address comes out of the table as an integer: say that it is global memory (a global, not a flat store)
  T* op = out + ((size_t)plane * ph + row) * pw + col;
  if constexpr (sizeof(T) == 4)
    *(__attribute__((address_space(1))) f32x4*)op = o;
  else
    *(__attribute__((address_space(1))) u32x2_t*)op = u32x2_t{pack_bf16x2(o.x, o.y), pack_bf16x2(o.z, o.w)};
}

// anchors [src_lo, src_lo + n) of y [B][4+nc][A] -> anchors [dst, dst + n) of cat [B][4+nc][A_tot]; blockIdx.y = image
__global__ __launch_bounds__(256) void tta_merge_kernel(const float* __restrict__ y, int nc, int A, int src_lo, int n,
                                                        float* __restrict__ cat, int A_tot, int dst, float scale,
                                                        int flip, float img_w, float img_h) {
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= n) return;
  const int no = 4 + nc;
  const float* in = y + (size_t)blockIdx.y * no * A + src_lo + a;
  float* out = cat + (size_t)blockIdx.y * no * A_tot + dst + a;
  float bx = in[0] / scale, by = in[A] / scale;
  const float bw = in[2 * (size_t)A] / scale, bh = in[3 * (size_t)A] / scale;
  if (flip == 3) bx = img_w - bx;
  if (flip == 2) by = img_h - by;
  out[0] = bx;
  out[A_tot] = by;
  out[2 * (size_t)A_tot] = bw;
  out[3 * (size_t)A_tot] = bh;
  const float* sp = in + 4 * (size_t)A;
  float* op = out + 4 * (size_t)A_tot;
  int c = 0;
  for (; c + 4 <= nc; c += 4) {  // four class rows in flight per lane
    float s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = sp[(size_t)(c + k) * A];
#pragma unroll
    for (int k = 0; k < 4; ++k) op[(size_t)(c + k) * A_tot] = s[k];
  }
#pragma clang loop vectorize(disable)
  for (; c < nc; ++c) op[(size_t)c * A_tot] = sp[(size_t)c * A];
}

}  // namespace ys

using namespace ys;

YS_EXPORT int yolosod_tta_views(const void* x, int B, int C, int H, int W, int bf16, const int64_t* desc, int V,
                                int max_ph, int max_pw, void* stream) {
  using namespace tta;
  YS_CHECK_ARG(x && desc, "tta_views: null pointer");
  YS_CHECK_ARG(B >= 1 && C >= 1 && H >= 1 && W >= 1 && H <= MAXDIM && W <= MAXDIM,
               "tta_views: x [%d, %d, %d, %d] unsupported (extents 1..%d)", B, C, H, W, MAXDIM);
  YS_CHECK_ARG(bf16 == 0 || bf16 == 1, "tta_views: bf16=%d", bf16);
  YS_CHECK_ARG(V >= 1 && (double)V * B * C <= 65535.0, "tta_views: V * B * C = %d * %d * %d unsupported (1..65535)", V,
               B, C);
  YS_CHECK_ARG(max_ph >= 1 && max_pw >= 4 && max_pw % 4 == 0 && max_ph <= MAXDIM && max_pw <= MAXDIM,
               "tta_views: padded size %dx%d unsupported (width %% 4 == 0, extents <= %d)", max_ph, max_pw, MAXDIM);
  YS_CHECK_ARG(((uintptr_t)desc & 7) == 0 && ((uintptr_t)x & (bf16 ? 1 : 3)) == 0, "tta_views: misaligned pointer");
  const dim3 grid((unsigned)((max_pw + TW - 1) / TW), (unsigned)((max_ph + TH - 1) / TH), (unsigned)(V * B * C));
  hipStream_t st = (hipStream_t)stream;
  if (bf16)
    hipLaunchKernelGGL(tta_views_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)x, B * C, H, W, desc, V, max_ph,
                       max_pw);
  else
    hipLaunchKernelGGL(tta_views_kernel<float>, grid, dim3(256), 0, st, (const float*)x, B * C, H, W, desc, V, max_ph,
                       max_pw);
  YS_CHECK_LAUNCH("tta_views");
  return 0;
}

YS_EXPORT int yolosod_tta_merge(const float* y, int B, int nc, int A, int src_lo, int n, float* cat, int A_tot, int dst,
                                float scale, int flip, float img_w, float img_h, void* stream) {
  YS_CHECK_ARG(y && cat, "tta_merge: null pointer");
  YS_CHECK_ARG(B >= 1 && B <= 65535, "tta_merge: B=%d unsupported (1..65535)", B);
  YS_CHECK_ARG(nc >= 1 && nc <= 64, "tta_merge: nc=%d unsupported (1..64)", nc);
  YS_CHECK_ARG(A >= 1 && A_tot >= 1, "tta_merge: A=%d, A_tot=%d", A, A_tot);
  YS_CHECK_ARG((double)A_tot * (4 + nc) < 2147483648.0 && (double)A * (4 + nc) < 2147483648.0,
               "tta_merge: A * (4 + nc) >= 2^31");
  YS_CHECK_ARG(n >= 1 && src_lo >= 0 && (long)src_lo + n <= A, "tta_merge: source anchors [%d, %d + %d) leave y's %d",
               src_lo, src_lo, n, A);
  YS_CHECK_ARG(dst >= 0 && (long)dst + n <= A_tot, "tta_merge: destination anchors [%d, %d + %d) leave cat's %d", dst,
               dst, n, A_tot);
  YS_CHECK_ARG(scale > 0.f && scale < __builtin_inff(), "tta_merge: scale must be finite and > 0");
  YS_CHECK_ARG(flip == 0 || flip == 2 || flip == 3, "tta_merge: flip=%d (0, 2 or 3)", flip);
  YS_CHECK_ARG(!(img_w != img_w) && !(img_h != img_h), "tta_merge: image size is NaN");
  YS_CHECK_ARG(((uintptr_t)y & 3) == 0 && ((uintptr_t)cat & 3) == 0, "tta_merge: misaligned pointer");
  const dim3 grid((unsigned)((n + 255) / 256), (unsigned)B);
  hipLaunchKernelGGL(tta_merge_kernel, grid, dim3(256), 0, (hipStream_t)stream, y, nc, A, src_lo, n, cat, A_tot, dst,
                     scale, flip, img_w, img_h);
  YS_CHECK_LAUNCH("tta_merge");
  return 0;
}
