// The front door: a batch of raw uint8 HWC BGR frames of any size -> the model's input tensor [B][3][out_h][out_w]
// (RGB planes, fp32 or bf16, values / 255, letterboxed onto a pad_value border) in one launch, and the padded NMS
// output mapped back to each frame's own pixels in one more (engine/predictor.py:116-134 non-tensor branch +
// LetterBox; models/yolo/detect/predict.py:23-41 + utils/ops.py:92-128).
//
// Written with torch ops the ingest is about eight full-resolution passes per frame (interpolate, pad, flip, permute,
// contiguous, float, div, stack) and a Python loop over frames of different sizes. Here one workgroup makes a 16 x 64
// output tile of one frame: the frame's descriptor (address, size, pitch, letterbox geometry) is read with uniform
// loads (one frame per blockIdx.z), the tile's axis maps (source index + 11-bit coefficient per output column / row:
// one integer division per thread) go to LDS, the source row segments the tile reads are staged in LDS with aligned
// dword loads (a BGR row starts at any byte address: 3 w is no multiple of 4 in general, and a frame may be a cropped
// view), and every lane then produces four consecutive output pixels of the three planes (16-byte stores) from bytes
// extracted out of LDS dwords (v_alignbyte). Only the source rows the tile's output rows touch are staged: a 3x
// down-scale reads two of every three source rows.
//
// The resize is defined in integers (cv2 INTER_LINEAR geometry: half-pixel centres, edge replicate, no antialias;
// 11-bit coefficients, one rounding), so it has one result on every machine; tests/ingest_ref.py restates it in numpy:
//   num = (2 d + 1) n - m, den = 2 m;  num < 0: s = 0, a = 0;  else s = num / den, a = ((num % den) 2048 + m) / den;
//   s >= n - 1: s = n - 1, a = 0;  s1 = min(s + 1, n - 1)
//   q = ((2048-ax)(2048-ay) p[y][x] + ax (2048-ay) p[y][x1] + (2048-ax) ay p[y1][x] + ax ay p[y1][x1] + 2^21) >> 22
// and the stored value is float(q) / 255.0f (an IEEE division: bit-equal to uint8 -> .float() / 255 on the CPU),
// rounded once more to nearest even for bf16. Everything fits 32 bits for extents <= 16384. a != 0 implies
// s1 = s + 1, so a tap pair is always read as the 6 consecutive bytes at s (the second pixel has weight 0 otherwise).
// Deterministic: no atomics, every output element written by exactly one lane.
#include "common.h"

namespace ys {

namespace ingest {
constexpr int TH = 16;             // output rows per tile
constexpr int TW = 64;             // output columns per tile (16 lanes x 4 pixels)
constexpr int SLOTS = 2 * TH;      // staged source rows per tile at most
constexpr int LDS_DW = 10112;      // staging dwords (with the two maps just under 40 KiB: four workgroups per CU)
constexpr int MAXDIM = 16384;      // source extents (14-bit index field; 32-bit arithmetic)
constexpr uint32_t VALID = 1u << 26;
}  // namespace ingest

// axis map entry of destination index d (extent m) onto a source of extent n: s | a << 14 | VALID; 0 outside [0, m)
__device__ __forceinline__ uint32_t axis_entry(int d, int n, int m) {
  if (d < 0 || d >= m) return 0u;
  const int num = (2 * d + 1) * n - m, den = 2 * m;
  int s = 0, a = 0;
  if (num >= 0) {
    s = num / den;
    a = ((num - s * den) * 2048 + m) / den;
  }
  if (s >= n - 1) {
    s = n - 1;
    a = 0;
  }
  return (uint32_t)s | ((uint32_t)a << 14) | ingest::VALID;
}

// bytes [off, off + 8) of an LDS row image as two dwords (off + 10 <= 4 * row dwords)
__device__ __forceinline__ uint2 lds_bytes8(const uint32_t* row, int off) {
  const uint32_t* p = row + (off >> 2);
  const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
  const uint32_t sh = (uint32_t)off & 3u;
  return make_uint2(__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh));
}

// the three channel results (B, G, R) of one output pixel from its four taps, each tap pair = 6 bytes (x, x + 1)
__device__ __forceinline__ void bilinear3(uint2 r0, uint2 r1, uint32_t ax, uint32_t ay, uint32_t* q) {
  const uint32_t w00 = (2048u - ax) * (2048u - ay), w01 = ax * (2048u - ay), w10 = (2048u - ax) * ay, w11 = ax * ay;
  const uint32_t a0[3] = {r0.x & 255u, (r0.x >> 8) & 255u, (r0.x >> 16) & 255u};
  const uint32_t a1[3] = {r0.x >> 24, r0.y & 255u, (r0.y >> 8) & 255u};
  const uint32_t b0[3] = {r1.x & 255u, (r1.x >> 8) & 255u, (r1.x >> 16) & 255u};
  const uint32_t b1[3] = {r1.x >> 24, r1.y & 255u, (r1.y >> 8) & 255u};
#pragma unroll
  for (int c = 0; c < 3; ++c) q[c] = (w00 * a0[c] + w01 * a1[c] + w10 * b0[c] + w11 * b1[c] + (1u << 21)) >> 22;
}

// desc [B][8] int64: source address, h, w, row pitch (bytes), new_h, new_w, top, left
template <class T>
__global__ __launch_bounds__(256) void letterbox_ingest_kernel(const int64_t* __restrict__ desc, T* __restrict__ out,
                                                               long out_bstride, int out_h, int out_w, float padv) {
  using namespace ingest;
  __shared__ __attribute__((aligned(16))) uint32_t xtab[TW];
  __shared__ uint32_t ytab[TH];
  __shared__ __attribute__((aligned(16))) uint32_t stage[LDS_DW];
  const int tid = threadIdx.x;
  const int b = blockIdx.z;
  const int64_t* dsc = desc + 8 * (size_t)b;  // uniform loads: one frame per blockIdx.z
  const uint8_t* src = (const uint8_t*)(uintptr_t)dsc[0];
  const int h = (int)dsc[1], w = (int)dsc[2];
  const long pitch = (long)dsc[3];
  const int nh = (int)dsc[4], nw = (int)dsc[5], top = (int)dsc[6], left = (int)dsc[7];

  const int r0 = blockIdx.y * TH, c0 = blockIdx.x * TW;
  const int ry = tid >> 4, xq = tid & 15;
  const int orow = r0 + ry, ocol = c0 + 4 * xq;
  const bool inb = orow < out_h && ocol < out_w;  // out_w % 4 == 0: a lane's four pixels are inside or outside together
  const size_t HW = (size_t)out_h * out_w;
  T* op = out + (size_t)b * out_bstride + (size_t)orow * out_w + ocol;
  const f32x4 pad4 = {padv, padv, padv, padv};

  // the tile's columns / rows inside the resized frame [left, left + nw) x [top, top + nh)
  const int cf = max(c0, left), cl = min(min(c0 + TW, left + nw), out_w) - 1;
  const int rf = max(r0, top), rl = min(min(r0 + TH, top + nh), out_h) - 1;
  if (cf > cl || rf > rl || h < 1 || w < 1) {  // border only
    if (inb) {
      st4(op, pad4);
      st4(op + HW, pad4);
      st4(op + 2 * HW, pad4);
    }
    return;
  }
  if (tid < TW) xtab[tid] = axis_entry(c0 + tid - left, w, nw);
  else if (tid < TW + TH) ytab[tid - TW] = axis_entry(r0 + (tid - TW) - top, h, nh);
  __syncthreads();

  // source columns [xs_lo, xs_hi] and rows [ys_lo, ys_hi] the tile reads (the maps are monotonic)
  const int xs_lo = (int)(xtab[cf - c0] & 0x3fffu), xs_hi = min((int)(xtab[cl - c0] & 0x3fffu) + 1, w - 1);
  const int ys_lo = (int)(ytab[rf - r0] & 0x3fffu), ys_hi = min((int)(ytab[rl - r0] & 0x3fffu) + 1, h - 1);
  const int ncols = xs_hi - xs_lo + 1;
  // LDS row image: the aligned dwords holding bytes [3 xs_lo, 3 (xs_hi + 1)) of a source row (at most
  // ((3 ncols + 2) >> 2) + 1 with the row's misalignment in front) + 2 dwords an 8-byte extraction may run over
  const int stride = ((3 * ncols + 2) >> 2) + 3;
  // staged rows: the contiguous range when it is short (up-scales, mild down-scales: neighbouring output rows share
  // source rows), else the two rows of each output row (slot 2 r + tap)
  const int span = ys_hi - ys_lo + 1;
  const bool contig = span <= SLOTS;
  const int nrows = contig ? span : SLOTS;
  const bool use_lds = nrows * stride <= LDS_DW;
  const uint8_t* col0 = src + 3 * (long)xs_lo;

  if (use_lds) {
    const int wv = tid >> 6, lane = tid & 63;
    const uint32_t* rbase[SLOTS / 4];
    int rnd[SLOTS / 4];
#pragma unroll
    for (int jj = 0; jj < SLOTS / 4; ++jj) {
      const int j = wv + 4 * jj;
      int srow = ys_lo + j;
      bool ok = j < nrows;
      if (!contig) {
        const uint32_t e = ytab[j >> 1];
        ok = (e & VALID) != 0u;
        srow = min((int)(e & 0x3fffu) + (j & 1), h - 1);
      }
      srow = ok ? srow : ys_lo;
      const uint8_t* a = col0 + (long)srow * pitch;
      const int mis = (int)((uintptr_t)a & 3u);
      rbase[jj] = (const uint32_t*)(a - mis);
      rnd[jj] = ok ? ((mis + 3 * ncols - 1) >> 2) + 1 : 0;  // every dword loaded holds a byte of the segment
    }
    for (int k = lane; k < stride - 2; k += 64) {
      uint32_t v[SLOTS / 4];
#pragma unroll
      for (int jj = 0; jj < SLOTS / 4; ++jj) v[jj] = k < rnd[jj] ? rbase[jj][k] : 0u;
#pragma unroll
      for (int jj = 0; jj < SLOTS / 4; ++jj)
        if (k < rnd[jj]) stage[(wv + 4 * jj) * stride + k] = v[jj];
    }
    __syncthreads();
  }
  if (!inb) return;

  const uint32_t ye = ytab[ry];
  f32x4 o[3] = {pad4, pad4, pad4};  // B, G, R
  if (ye & VALID) {
    const int sy = (int)(ye & 0x3fffu), sy1 = min(sy + 1, h - 1);
    const uint32_t ay = (ye >> 14) & 0xfffu;
    const u32x4_t xe4 = *reinterpret_cast<const u32x4_t*>(&xtab[4 * xq]);
    const uint32_t xe[4] = {xe4.x, xe4.y, xe4.z, xe4.w};
    const uint8_t* g0 = col0 + (long)sy * pitch;
    const uint8_t* g1 = col0 + (long)sy1 * pitch;
    if (use_lds) {
      const int slot0 = contig ? sy - ys_lo : 2 * ry;
      const int slot1 = contig ? min(slot0 + 1, nrows - 1) : slot0 + 1;
      const uint32_t* l0 = stage + slot0 * stride;
      const uint32_t* l1 = stage + slot1 * stride;
      const int m0 = (int)((uintptr_t)g0 & 3u), m1 = (int)((uintptr_t)g1 & 3u);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int sx = min(max((int)(xe[j] & 0x3fffu), xs_lo), xs_hi) - xs_lo;  // border pixels read column xs_lo
        const uint32_t ax = (xe[j] >> 14) & 0xfffu;
        uint32_t q[3];
        bilinear3(lds_bytes8(l0, m0 + 3 * sx), lds_bytes8(l1, m1 + 3 * sx), ax, ay, q);
        if (xe[j] & VALID) {
          o[0][j] = (float)q[0] / 255.0f;
          o[1][j] = (float)q[1] / 255.0f;
          o[2][j] = (float)q[2] / 255.0f;
        }
      }
    } else {
      // a tile whose source window does not fit the staging block (down-scales beyond ~6x): the taps straight from
      // global memory, byte by byte
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!(xe[j] & VALID)) continue;
        const int sx = (int)(xe[j] & 0x3fffu), sx1 = min(sx + 1, w - 1);
        const uint32_t ax = (xe[j] >> 14) & 0xfffu;
        const long o0 = 3 * (long)(sx - xs_lo), o1 = 3 * (long)(sx1 - xs_lo);
        const uint2 t0 = make_uint2((uint32_t)g0[o0] | ((uint32_t)g0[o0 + 1] << 8) | ((uint32_t)g0[o0 + 2] << 16) |
                                        ((uint32_t)g0[o1] << 24),
                                    (uint32_t)g0[o1 + 1] | ((uint32_t)g0[o1 + 2] << 8));
        const uint2 t1 = make_uint2((uint32_t)g1[o0] | ((uint32_t)g1[o0 + 1] << 8) | ((uint32_t)g1[o0 + 2] << 16) |
                                        ((uint32_t)g1[o1] << 24),
                                    (uint32_t)g1[o1 + 1] | ((uint32_t)g1[o1 + 2] << 8));
        uint32_t q[3];
        bilinear3(t0, t1, ax, ay, q);
        o[0][j] = (float)q[0] / 255.0f;
        o[1][j] = (float)q[1] / 255.0f;
        o[2][j] = (float)q[2] / 255.0f;
      }
    }
  }
  st4(op, o[2]);  // planes in RGB order
  st4(op + HW, o[1]);
  st4(op + 2 * HW, o[0]);
}

// det [B][D][6]: rows < counts[b]: (v - pad) / gain, clamped to the frame; geom [B][5] = gain, pad_x, pad_y, w0, h0
__global__ __launch_bounds__(256) void scale_boxes_kernel(float* __restrict__ det, const int* __restrict__ counts,
                                                          int B, int D, const float* __restrict__ geom) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * D) return;
  const int b = (int)(i / D), r = (int)(i - (long)b * D);
  if (r >= counts[b]) return;
  const float* g = geom + 5 * b;
  const float gain = g[0], px = g[1], py = g[2], w0 = g[3], h0 = g[4];
  float* v = det + 6 * i;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float t = (v[k] - ((k & 1) ? py : px)) / gain;  // IEEE division, as the CPU's boxes /= gain
    const float hi = (k & 1) ? h0 : w0;
    t = t < 0.f ? 0.f : t;  // clamp(0, hi) that keeps a NaN
    t = t > hi ? hi : t;
    v[k] = t;
  }
}

}  // namespace ys

using namespace ys;

YS_EXPORT int yolosod_letterbox_ingest(const int64_t* desc, int B, void* out, long out_bstride, int out_h, int out_w,
                                       int out_bf16, int pad_value, void* stream) {
  using namespace ingest;
  YS_CHECK_ARG(desc && out, "letterbox_ingest: null pointer");
  YS_CHECK_ARG(B >= 1 && B <= 65535, "letterbox_ingest: B=%d unsupported (1..65535)", B);
  YS_CHECK_ARG(out_h >= 1 && out_w >= 4 && out_w % 4 == 0 && out_h <= MAXDIM && out_w <= MAXDIM,
               "letterbox_ingest: canvas %dx%d unsupported (out_w %% 4 == 0, extents <= %d)", out_h, out_w, MAXDIM);
  YS_CHECK_ARG(out_bstride % 4 == 0 && out_bstride >= 3L * out_h * out_w,
               "letterbox_ingest: batch stride %ld must be a multiple of 4 and >= 3*out_h*out_w", out_bstride);
  YS_CHECK_ARG(((uintptr_t)out & 15) == 0 && ((uintptr_t)desc & 7) == 0, "letterbox_ingest: out must be 16-byte aligned");
  YS_CHECK_ARG(out_bf16 == 0 || out_bf16 == 1, "letterbox_ingest: out_bf16=%d", out_bf16);
  YS_CHECK_ARG(pad_value >= 0 && pad_value <= 255, "letterbox_ingest: pad_value=%d outside [0, 255]", pad_value);
  const float padv = (float)pad_value / 255.0f;
  const dim3 grid((unsigned)((out_w + TW - 1) / TW), (unsigned)((out_h + TH - 1) / TH), (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  if (out_bf16)
    hipLaunchKernelGGL(letterbox_ingest_kernel<bf16_t>, grid, dim3(256), 0, st, desc, (bf16_t*)out, out_bstride, out_h,
                       out_w, padv);
  else
    hipLaunchKernelGGL(letterbox_ingest_kernel<float>, grid, dim3(256), 0, st, desc, (float*)out, out_bstride, out_h,
                       out_w, padv);
  YS_CHECK_LAUNCH("letterbox_ingest");
  return 0;
}

YS_EXPORT int yolosod_scale_boxes(float* det, const int* counts, int B, int D, const float* geom, void* stream) {
  YS_CHECK_ARG(det && counts && geom, "scale_boxes: null pointer");
  YS_CHECK_ARG(B >= 1, "scale_boxes: B=%d", B);
  YS_CHECK_ARG(D >= 1 && D <= (1 << 20), "scale_boxes: D=%d unsupported (1..2^20)", D);
  const long rows = (long)B * D;
  YS_CHECK_ARG((rows + 255) / 256 < (1L << 31), "scale_boxes: too many rows");
  hipLaunchKernelGGL(scale_boxes_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, det,
                     counts, B, D, geom);
  YS_CHECK_LAUNCH("scale_boxes");
  return 0;
}
