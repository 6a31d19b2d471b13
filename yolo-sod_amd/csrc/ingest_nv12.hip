// The front door for decoded video: a batch of NV12 surfaces (a full-resolution Y plane and a half-resolution
// interleaved UV plane, each with its own row pitch; what a hardware video decoder writes) of any size -> the model's
// input tensor [B][3][out_h][out_w] (RGB planes, fp32 or bf16, values / 255, letterboxed onto a pad_value border) in
// one launch. The project's own: the reference reads BGR frames only (csrc/ingest.hip is that path and stays as it is).
//
// Definition: ingest_nv12(frames) == ingest_bgr(nv12_to_bgr_u8(frames)) bit for bit. View pixel (r, c) of a frame
// takes Y[r][c] and the chroma pair UV[(r + py) >> 1][(c + px) >> 1] (replicated over its 2 x 2 block, no chroma
// interpolation; py, px are the parities of the view's origin on its surface: a tile of a sliced frame starts
// anywhere) and becomes uint8 B, G, R in int32 arithmetic (arithmetic right shift, saturation to [0, 255]):
//   y = max(Y - YOFF, 0) CY;  u = U - 128;  v = V - 128
//   R = sat((y + CVR v + 2^19) >> 20);  G = sat((y + CVG v + CUG u + 2^19) >> 20);  B = sat((y + CUB u + 2^19) >> 20)
// with one of four coefficient rows per frame (nv12::COEF; |accumulator| <= 573,487,137 over all 2^24 triples). The
// converted pixels then go through csrc/ingest.hip's integer bilinear, restated here unchanged (axis_entry,
// lds_bytes8, bilinear3): same axis maps, 11-bit coefficients, one rounding, float(q) / 255.0f, bf16 rounded once.
// tests/nv12_ref.py restates the conversion in numpy int64.
//
// One workgroup makes a 16 x 64 output tile of one frame (uniform descriptor loads, one frame per blockIdx.z). The
// source window of the tile is converted ONCE into an LDS image of 3-byte BGR pixels (row j, pixel k at byte 3 k: the
// image is aligned whatever the surface's addresses are), four pixels per work item: the aligned dwords that hold its
// 4 Y bytes (<= 2) and its 2..3 chroma pairs (<= 3) are loaded, the bytes extracted (v_alignbyte), the chroma terms
// computed once per pair, and 12 bytes stored. Only dwords that hold a byte of the window are loaded: nothing outside
// the surface is touched. The tap path on the image is the BGR kernel's. Staged rows as there: the contiguous source
// row range when it spans at most 32 rows, else the two rows of each output row; a window that does not fit the block
// (down-scales beyond ~6x) converts per tap from global memory, byte by byte. Deterministic: no atomics, every
// output element written by exactly one lane.
#include "common.h"

namespace ys {

namespace nv12 {
constexpr int TH = 16;             // output rows per tile
constexpr int TW = 64;             // output columns per tile (16 lanes x 4 pixels)
constexpr int SLOTS = 2 * TH;      // staged source rows per tile at most
constexpr int LDS_DW = 10112;      // BGR image dwords (with the two maps just under 40 KiB: four workgroups per CU)
constexpr int MAXDIM = 16384;      // source extents (14-bit index field; 32-bit arithmetic)
constexpr int DESC = 12;           // int64 fields per frame
constexpr uint32_t VALID = 1u << 26;
// YOFF, CY, CVR, CUG, CVG, CUB: bt601, bt709 (limited range), bt601_full, bt709_full. The three-decimal textbook
// constants times 2^20, rounded half away from zero (yolo-sod_amd/data/nv12.py holds the same table).
__constant__ int COEF[4][6] = {{16, 1220542, 1673527, -409993, -852492, 2116026},
                               {16, 1220542, 1880097, -223347, -558891, 2214593},
                               {0, 1048576, 1470104, -360710, -748683, 1858077},
                               {0, 1048576, 1651507, -196084, -490734, 1946157}};
struct Matrix {
  int yoff, cy, cvr, cug, cvg, cub;
};
}  // namespace nv12

// axis map entry of destination index d (extent m) onto a source of extent n: s | a << 14 | VALID; 0 outside [0, m)
__device__ __forceinline__ uint32_t nv12_axis_entry(int d, int n, int m) {
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
  return (uint32_t)s | ((uint32_t)a << 14) | nv12::VALID;
}

// bytes [off, off + 8) of an LDS row image as two dwords (off + 10 <= 4 * row dwords)
__device__ __forceinline__ uint2 nv12_lds_bytes8(const uint32_t* row, int off) {
  const uint32_t* p = row + (off >> 2);
  const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
  const uint32_t sh = (uint32_t)off & 3u;
  return make_uint2(__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh));
}

// the three channel results (B, G, R) of one output pixel from its four taps, each tap pair = 6 bytes (x, x + 1)
__device__ __forceinline__ void nv12_bilinear3(uint2 r0, uint2 r1, uint32_t ax, uint32_t ay, uint32_t* q) {
  const uint32_t w00 = (2048u - ax) * (2048u - ay), w01 = ax * (2048u - ay), w10 = (2048u - ax) * ay, w11 = ax * ay;
  const uint32_t a0[3] = {r0.x & 255u, (r0.x >> 8) & 255u, (r0.x >> 16) & 255u};
  const uint32_t a1[3] = {r0.x >> 24, r0.y & 255u, (r0.y >> 8) & 255u};
  const uint32_t b0[3] = {r1.x & 255u, (r1.x >> 8) & 255u, (r1.x >> 16) & 255u};
  const uint32_t b1[3] = {r1.x >> 24, r1.y & 255u, (r1.y >> 8) & 255u};
#pragma unroll
  for (int c = 0; c < 3; ++c) q[c] = (w00 * a0[c] + w01 * a1[c] + w10 * b0[c] + w11 * b1[c] + (1u << 21)) >> 22;
}

__device__ __forceinline__ int nv12_sat8(int v) { return min(max(v, 0), 255); }

// the chroma terms of one pair (U in the low byte, V in the next): added to a pixel's luma term they give R, G, B
__device__ __forceinline__ void nv12_chroma(uint32_t uv, const nv12::Matrix& m, int& tr, int& tg, int& tb) {
  const int u = (int)(uv & 255u) - 128, v = (int)((uv >> 8) & 255u) - 128;
  tr = m.cvr * v;
  tg = m.cvg * v + m.cug * u;
  tb = m.cub * u;
}

// one pixel as B | G << 8 | R << 16
__device__ __forceinline__ uint32_t nv12_pixel(uint32_t Y, int tr, int tg, int tb, const nv12::Matrix& m) {
  const int y = max((int)Y - m.yoff, 0) * m.cy + (1 << 19);
  return (uint32_t)nv12_sat8((y + tb) >> 20) | ((uint32_t)nv12_sat8((y + tg) >> 20) << 8) |
         ((uint32_t)nv12_sat8((y + tr) >> 20) << 16);
}

// view pixel (row pointers yrow / uvrow of its Y row and chroma row, column c) from global memory, byte by byte
__device__ __forceinline__ uint32_t nv12_pixel_global(const uint8_t* yrow, const uint8_t* uvrow, int c, int px,
                                                      const nv12::Matrix& m) {
  const uint8_t* p = uvrow + 2 * ((c + px) >> 1);
  int tr, tg, tb;
  nv12_chroma((uint32_t)p[0] | ((uint32_t)p[1] << 8), m, tr, tg, tb);
  return nv12_pixel(yrow[c], tr, tg, tb, m);
}

// desc [B][12] int64: Y address of the view's first pixel, UV address of that pixel's chroma pair, h, w, Y pitch,
// UV pitch (bytes), new_h, new_w, top, left, origin parities (y0 & 1) << 1 | (x0 & 1), matrix id
template <class T>
__global__ __launch_bounds__(256) void letterbox_ingest_nv12_kernel(const int64_t* __restrict__ desc,
                                                                    T* __restrict__ out, long out_bstride, int out_h,
                                                                    int out_w, float padv) {
  using namespace nv12;
  __shared__ __attribute__((aligned(16))) uint32_t xtab[TW];
  __shared__ uint32_t ytab[TH];
  __shared__ __attribute__((aligned(16))) uint32_t stage[LDS_DW];
  const int tid = threadIdx.x;
  const int b = blockIdx.z;
  const int64_t* dsc = desc + DESC * (size_t)b;  // uniform loads: one frame per blockIdx.z
  const uint8_t* ysrc = (const uint8_t*)(uintptr_t)dsc[0];
  const uint8_t* uvsrc = (const uint8_t*)(uintptr_t)dsc[1];
  const int h = (int)dsc[2], w = (int)dsc[3];
  const long ypitch = (long)dsc[4], uvpitch = (long)dsc[5];
  const int nh = (int)dsc[6], nw = (int)dsc[7], top = (int)dsc[8], left = (int)dsc[9];
  const int py = ((int)dsc[10] >> 1) & 1, px = (int)dsc[10] & 1;
  const int* cf6 = COEF[(int)dsc[11] & 3];
  const Matrix mat = {cf6[0], cf6[1], cf6[2], cf6[3], cf6[4], cf6[5]};

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
  if (tid < TW) xtab[tid] = nv12_axis_entry(c0 + tid - left, w, nw);
  else if (tid < TW + TH) ytab[tid - TW] = nv12_axis_entry(r0 + (tid - TW) - top, h, nh);
  __syncthreads();

  // source columns [xs_lo, xs_hi] and rows [ys_lo, ys_hi] the tile reads (the maps are monotonic)
  const int xs_lo = (int)(xtab[cf - c0] & 0x3fffu), xs_hi = min((int)(xtab[cl - c0] & 0x3fffu) + 1, w - 1);
  const int ys_lo = (int)(ytab[rf - r0] & 0x3fffu), ys_hi = min((int)(ytab[rl - r0] & 0x3fffu) + 1, h - 1);
  const int ncols = xs_hi - xs_lo + 1;
  // LDS row image: groups of four pixels (3 dwords each) + 2 dwords an 8-byte extraction may run over
  const int groups = (ncols + 3) >> 2;
  const int stride = 3 * groups + 2;
  // staged rows: the contiguous range when it is short (up-scales, mild down-scales: neighbouring output rows share
  // source rows), else the two rows of each output row (slot 2 r + tap)
  const int span = ys_hi - ys_lo + 1;
  const bool contig = span <= SLOTS;
  const int nrows = contig ? span : SLOTS;
  const bool use_lds = nrows * stride <= LDS_DW;

  if (use_lds) {
    for (int it = tid; it < nrows * groups; it += 256) {
      const int j = it / groups, g = it - j * groups;
      int srow = ys_lo + j;
      if (!contig) {
        const uint32_t e = ytab[j >> 1];
        if (!(e & VALID)) continue;  // an output row outside the resized frame: its two slots are never read
        srow = min((int)(e & 0x3fffu) + (j & 1), h - 1);
      }
      const int col = xs_lo + 4 * g;             // first view column of the group
      const int nv = min(4, xs_hi + 1 - col);    // its pixels inside the window (1..4)
      // Y: bytes [a, a + nv)
      const uint8_t* a = ysrc + (long)srow * ypitch + col;
      const uint32_t my = (uint32_t)((uintptr_t)a & 3u);
      const uint32_t* ya = (const uint32_t*)(a - my);
      const uint32_t y0 = ya[0];
      const uint32_t y1 = (int)my + nv > 4 ? ya[1] : 0u;  // every dword loaded holds a byte of the window
      const uint32_t yy = __builtin_amdgcn_alignbyte(y1, y0, my);
      // chroma: pairs [p0, p0 + np) of the chroma row, bytes [u, u + 2 np)
      const int cg = col + px, p0 = cg >> 1;
      const int np = ((cg + nv - 1) >> 1) - p0 + 1;  // 1..3
      const uint8_t* u = uvsrc + (long)((srow + py) >> 1) * uvpitch + 2 * (long)p0;
      const uint32_t mu = (uint32_t)((uintptr_t)u & 3u);
      const uint32_t* ua = (const uint32_t*)(u - mu);
      const uint32_t e0 = ua[0];
      const uint32_t e1 = (int)mu + 2 * np > 4 ? ua[1] : 0u;
      const uint32_t e2 = (int)mu + 2 * np > 8 ? ua[2] : 0u;
      const uint32_t c01 = __builtin_amdgcn_alignbyte(e1, e0, mu), c2 = __builtin_amdgcn_alignbyte(e2, e1, mu);
      int tr[3], tg[3], tb[3];
      nv12_chroma(c01 & 0xffffu, mat, tr[0], tg[0], tb[0]);
      nv12_chroma(c01 >> 16, mat, tr[1], tg[1], tb[1]);
      nv12_chroma(c2 & 0xffffu, mat, tr[2], tg[2], tb[2]);
      // pixel i takes pair (i + (cg & 1)) >> 1: an even group start 0 0 1 1, an odd one 0 1 1 2
      const bool odd = cg & 1;
      const int k1 = odd ? 1 : 0, k3 = odd ? 2 : 1;
      const uint32_t q0 = nv12_pixel(yy & 255u, tr[0], tg[0], tb[0], mat);
      const uint32_t q1 = nv12_pixel((yy >> 8) & 255u, tr[k1], tg[k1], tb[k1], mat);
      const uint32_t q2 = nv12_pixel((yy >> 16) & 255u, tr[1], tg[1], tb[1], mat);
      const uint32_t q3 = nv12_pixel(yy >> 24, tr[k3], tg[k3], tb[k3], mat);
      uint32_t* d = stage + j * stride + 3 * g;  // pixels past the window hold defined bytes nobody weighs
      d[0] = q0 | (q1 << 24);
      d[1] = (q1 >> 8) | (q2 << 16);
      d[2] = (q2 >> 16) | (q3 << 8);
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
    if (use_lds) {
      const int slot0 = contig ? sy - ys_lo : 2 * ry;
      const int slot1 = contig ? min(slot0 + 1, nrows - 1) : slot0 + 1;
      const uint32_t* l0 = stage + slot0 * stride;
      const uint32_t* l1 = stage + slot1 * stride;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int sx = min(max((int)(xe[j] & 0x3fffu), xs_lo), xs_hi) - xs_lo;  // border pixels read column xs_lo
        const uint32_t ax = (xe[j] >> 14) & 0xfffu;
        uint32_t q[3];
        nv12_bilinear3(nv12_lds_bytes8(l0, 3 * sx), nv12_lds_bytes8(l1, 3 * sx), ax, ay, q);
        if (xe[j] & VALID) {
          o[0][j] = (float)q[0] / 255.0f;
          o[1][j] = (float)q[1] / 255.0f;
          o[2][j] = (float)q[2] / 255.0f;
        }
      }
    } else {
      // a tile whose source window does not fit the staging block (down-scales beyond ~6x): the four taps converted
      // straight from global memory, byte by byte
      const uint8_t* g0 = ysrc + (long)sy * ypitch;
      const uint8_t* g1 = ysrc + (long)sy1 * ypitch;
      const uint8_t* u0 = uvsrc + (long)((sy + py) >> 1) * uvpitch;
      const uint8_t* u1 = uvsrc + (long)((sy1 + py) >> 1) * uvpitch;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!(xe[j] & VALID)) continue;
        const int sx = (int)(xe[j] & 0x3fffu), sx1 = min(sx + 1, w - 1);
        const uint32_t ax = (xe[j] >> 14) & 0xfffu;
        const uint32_t p00 = nv12_pixel_global(g0, u0, sx, px, mat), p01 = nv12_pixel_global(g0, u0, sx1, px, mat);
        const uint32_t p10 = nv12_pixel_global(g1, u1, sx, px, mat), p11 = nv12_pixel_global(g1, u1, sx1, px, mat);
        uint32_t q[3];
        nv12_bilinear3(make_uint2(p00 | (p01 << 24), p01 >> 8), make_uint2(p10 | (p11 << 24), p11 >> 8), ax, ay, q);
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

}  // namespace ys

using namespace ys;

YS_EXPORT int yolosod_letterbox_ingest_nv12(const int64_t* desc, int B, void* out, long out_bstride, int out_h,
                                            int out_w, int out_bf16, int pad_value, void* stream) {
  using namespace nv12;
  YS_CHECK_ARG(desc && out, "letterbox_ingest_nv12: null pointer");
  YS_CHECK_ARG(B >= 1 && B <= 65535, "letterbox_ingest_nv12: B=%d unsupported (1..65535)", B);
  YS_CHECK_ARG(out_h >= 1 && out_w >= 4 && out_w % 4 == 0 && out_h <= MAXDIM && out_w <= MAXDIM,
               "letterbox_ingest_nv12: canvas %dx%d unsupported (out_w %% 4 == 0, extents <= %d)", out_h, out_w, MAXDIM);
  YS_CHECK_ARG(out_bstride % 4 == 0 && out_bstride >= 3L * out_h * out_w,
               "letterbox_ingest_nv12: batch stride %ld must be a multiple of 4 and >= 3*out_h*out_w", out_bstride);
  YS_CHECK_ARG(((uintptr_t)out & 15) == 0 && ((uintptr_t)desc & 7) == 0,
               "letterbox_ingest_nv12: out must be 16-byte aligned");
  YS_CHECK_ARG(out_bf16 == 0 || out_bf16 == 1, "letterbox_ingest_nv12: out_bf16=%d", out_bf16);
  YS_CHECK_ARG(pad_value >= 0 && pad_value <= 255, "letterbox_ingest_nv12: pad_value=%d outside [0, 255]", pad_value);
  const float padv = (float)pad_value / 255.0f;
  const dim3 grid((unsigned)((out_w + TW - 1) / TW), (unsigned)((out_h + TH - 1) / TH), (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  if (out_bf16)
    hipLaunchKernelGGL(letterbox_ingest_nv12_kernel<bf16_t>, grid, dim3(256), 0, st, desc, (bf16_t*)out, out_bstride,
                       out_h, out_w, padv);
  else
    hipLaunchKernelGGL(letterbox_ingest_nv12_kernel<float>, grid, dim3(256), 0, st, desc, (float*)out, out_bstride,
                       out_h, out_w, padv);
  YS_CHECK_LAUNCH("letterbox_ingest_nv12");
  return 0;
}
