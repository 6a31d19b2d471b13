// bf16 model config: SwinBlock and A2_Attn with bf16 activations on the bf16 matrix cores (fp32 accumulation).
//
//   * gemm_bf16     - gemm_bf16.h: v_mfma_f32_32x32x16_bf16, LN prologue, bias / BN / act / residual epilogue.
//   * window_attn   - per-(sequence, head, 64 queries) attention on v_mfma_f32_16x16x32_bf16: K (row-major) and V
//                     (transposed) of the whole sequence in LDS, one wave per 16 queries, the full score row in
//                     registers (fp32 softmax, no rescaling), P through a per-wave LDS tile into the P.V product.
//   * swin_tokens   - depthwise 3x3 + bottom/right zero pad -> token-major rows in padded RASTER order
//                     [img][Hp][Wp][C]. Every Swin stage except attention is per token, so the window partition is
//                     only an index map inside the attention kernel, and the window reverse + crop of the output
//                     is a plain NCHW store of each token row (contiguous pixels).
//   * a2 pool / upsample - as transformer.hip, bf16 storage.
// Arithmetic: activations are bf16 in HBM (as `model.to(torch.bfloat16)` stores them); every reduction, LayerNorm,
// softmax and epilogue runs in fp32 and rounds once on store. Parameters other than the GEMM weights are fp32.
//
// Reference semantics (fp32 originals): SwinBlock blocks_transformer.py:8-171, A2_Attn a2_attn.py:35-69.
#include "common.h"
#include "gemm_bf16.h"
#include <math.h>
#include <stdlib.h>

namespace ys {

// token row of (sequence, token) in the attention's qkv / out matrices
struct TokMap {
  int mode;  // 0: row = seq * L + t;  1: Swin window (img, wy, wx) of a padded raster [img][Hp][Wp]
  int L, Hp, Wp, wh, ww, nWx, nWin;
  __device__ __forceinline__ long row(long seq, int t) const {
    if (mode == 0) return seq * L + t;
    const long img = seq / nWin;
    const int win = (int)(seq - img * nWin);
    const int wy = win / nWx, wx = win - (win / nWx) * nWx;
    const int iy = t / ww, ix = t - (t / ww) * ww;
    return (img * Hp + wy * wh + iy) * (long)Wp + wx * ww + ix;
  }
};

typedef short s16x8 __attribute__((ext_vector_type(8)));

// =================================================================================================
// Attention over packed bf16 QKV rows: q at col h*HD, k at C + h*HD, v at 2C + h*HD of a row of ld = 3C;
// out[row][h*HD + d]. grid = (ceil(L/64), heads, n_seq); 256 threads, wave w owns queries q0 + 16w .. +15.
// MFMA 16x16x32 bf16: A/B lane l holds [row l&15][k = 8(l>>4) + j]; C/D lane l holds [row 4(l>>4) + r][col l&15].
// S = Q K^T (fp32), softmax(S * scale) in fp32 with the row spread over the 16 lanes of a lane group, P rounded to
// bf16 (the reference bf16 model's P), O = P V. V is staged row-major like K (16-byte stores) and read transposed into
// the PV B operand with ds_read_b64_tr_b16: staging V^T with 2-byte stores had 16 lanes of one key on one bank
// (16-way conflicts; 74 % of the kernel's LDS cycles at L9_m). The 16-column blocks of the V rows with bit 3 set are
// XOR-swapped with the other half of the row (vcol), so the two key quads a 32-lane half reads (rows 8 apart) sit on
// disjoint banks.
// =================================================================================================
template <int HD>
__device__ __forceinline__ int vcol(int row, int col) {
  return (((col >> 4) ^ (((row >> 3) & 1) * (HD / 32))) << 4) | (col & 15);
}
template <int HD, int NKB>
__global__ __launch_bounds__(256) void window_attn_bf16_kernel(const bf16_t* __restrict__ qkv, int C,
                                                               bf16_t* __restrict__ out, TokMap tm, float scale) {
  constexpr int NK = NKB * 16;       // keys (padded)
  constexpr int KS = HD + 8;         // K row stride (elements)
  constexpr int VS = HD + 16;        // V row stride (keys are rows)
  constexpr int PS = NK + 8;         // P row stride
  static_assert(NK % 32 == 0 && HD % 32 == 0, "k steps of 32");
  __shared__ __attribute__((aligned(16))) bf16_t Ks[NK * KS];
  __shared__ __attribute__((aligned(16))) bf16_t Vr[NK * VS];
  __shared__ __attribute__((aligned(16))) bf16_t Ps[4 * 16 * PS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int h = blockIdx.y;
  const long seq = blockIdx.z;
  const int L = tm.L;
  const int ld = 3 * C;
  const int l15 = lane & 15, g = lane >> 4;

  // stage K and V (both row-major) of the sequence: every load of the thread first, then the LDS stores, with keys
  // >= L reading key L - 1 (finite; their scores are masked before the softmax and meet P = 0 in P.V). A predicated
  // load in the store loop waited for each load in turn.
  constexpr int NE = NK * (HD / 8), NR = (NE + 255) / 256;  // 16-byte items, staging rounds
  u32x4_t kv[NR], vv[NR];
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const int e = (tid + 256 * i < NE) ? tid + 256 * i : NE - 1;  // a partial last round re-reads the last item
    const int key = e / (HD / 8), dc = (e - key * (HD / 8)) * 8;
    const bf16_t* src = qkv + tm.row(seq, key < L ? key : L - 1) * ld + h * HD + dc;
    kv[i] = *reinterpret_cast<const u32x4_t*>(src + C);
    vv[i] = *reinterpret_cast<const u32x4_t*>(src + 2 * C);
  }
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const int e = tid + 256 * i;
    if (NE % 256 != 0 && e >= NE) break;
    const int key = e / (HD / 8), dc = (e - key * (HD / 8)) * 8;
    *reinterpret_cast<u32x4_t*>(&Ks[key * KS + dc]) = kv[i];
    *reinterpret_cast<u32x4_t*>(&Vr[key * VS + vcol<HD>(key, dc)]) = vv[i];
  }
  // this wave's Q fragments (rows >= L read row L-1: finite values, results dropped)
  const int q0 = blockIdx.x * 64 + wv * 16;
  bf16x8_t qf[HD / 32];
  {
    const int qr = (q0 + l15 < L) ? q0 + l15 : L - 1;
    const bf16_t* src = qkv + tm.row(seq, qr) * ld + h * HD + 8 * g;
#pragma unroll
    for (int s = 0; s < HD / 32; ++s) qf[s] = *reinterpret_cast<const bf16x8_t*>(src + 32 * s);
  }
  __syncthreads();
  if (q0 >= L) return;  // whole wave; no barrier below (the per-wave P tile is ordered by the wave barrier)

  f32x4 sacc[NKB];
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    const bf16_t* kr = Ks + (kb * 16 + l15) * KS + 8 * g;
#pragma unroll
    for (int s = 0; s < HD / 32; ++s)
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[s], *reinterpret_cast<const bf16x8_t*>(kr + 32 * s), a, 0, 0, 0);
    sacc[kb] = a;
  }
  // softmax over keys: lane holds S[row 4g + r][key kb*16 + l15]
  const float sl = scale * 1.44269504088896341f;  // exp(x*scale) = exp2(x*scale*log2 e)
  float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
    const bool valid = kb * 16 + l15 < L;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (!valid) sacc[kb][r] = -INFINITY;
      mx[r] = fmaxf(mx[r], sacc[kb][r]);
    }
  }
  float sum[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) mx[r] = fmaxf(mx[r], __shfl_xor(mx[r], o, 64));
    sum[r] = 0.f;
  }
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e = __builtin_amdgcn_exp2f((sacc[kb][r] - mx[r]) * sl);
      sacc[kb][r] = e;
      sum[r] += e;
    }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) sum[r] += __shfl_xor(sum[r], o, 64);
    sum[r] = 1.0f / sum[r];
  }
  bf16_t* Pw = Ps + wv * 16 * PS;
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r) Pw[(4 * g + r) * PS + kb * 16 + l15] = f2bf(sacc[kb][r] * sum[r]);
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's P stores are in LDS before its reads
  __builtin_amdgcn_wave_barrier();

  f32x4 oacc[HD / 16];
#pragma unroll
  for (int db = 0; db < HD / 16; ++db) oacc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  // transposed V reads: lane 4q + p of lane group g supplies row (key) 32s + 8g + q (+ 4), columns db*16 + 4p .. +3;
  // lane l15 receives column (d) db*16 + l15 of the 4 keys - the B operand's k slots 8g .. 8g + 3 (+ 4 .. 7)
  const int tq = l15 >> 2, tp = l15 & 3;
#pragma unroll
  for (int s = 0; s < NK / 32; ++s) {
    const bf16x8_t pa = *reinterpret_cast<const bf16x8_t*>(Pw + l15 * PS + 32 * s + 8 * g);
    const int r0 = 32 * s + 8 * g + tq;
#pragma unroll
    for (int db = 0; db < HD / 16; ++db) {
      typedef short s16x4 __attribute__((ext_vector_type(4)));
      typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
      const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_s16x4*)(Vr + r0 * VS + vcol<HD>(r0, db * 16 + 4 * tp)));
      const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_s16x4*)(Vr + (r0 + 4) * VS + vcol<HD>(r0 + 4, db * 16 + 4 * tp)));
      const s16x8 v8 = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
      oacc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, __builtin_bit_cast(bf16x8_t, v8), oacc[db], 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = q0 + 4 * g + r;
    if (q >= L) continue;
    bf16_t* dst = out + tm.row(seq, q) * C + h * HD + l15;
#pragma unroll
    for (int db = 0; db < HD / 16; ++db) dst[db * 16] = f2bf(oacc[db][r]);
  }
}

template <int HD, int N>
constexpr size_t wattn_lds_bytes() {
  return sizeof(bf16_t) * ((size_t)N * 16 * (HD + 8) + (size_t)N * 16 * (HD + 16) + 64 * (size_t)(N * 16 + 8));
}

// key-block counts with an instance whose K / V^T / P tiles fit the 160 KiB of LDS
#define YS_WATTN_ALL YS_WATTN(4) YS_WATTN(6) YS_WATTN(8) YS_WATTN(10) YS_WATTN(12) YS_WATTN(16) YS_WATTN(20)

// the instance (its NKB) that takes nkb key blocks of head dim HD; -1: none compiled
template <int HD>
static int wattn_instance(int nkb) {
#define YS_WATTN(N)                                               \
  if constexpr (wattn_lds_bytes<HD, N>() <= 160 * 1024) {         \
    if (nkb <= N) return N;                                       \
  }
  YS_WATTN_ALL
#undef YS_WATTN
  return -1;
}

static int wattn_key_blocks(int L) { return ((L + 31) / 32) * 2; }  // blocks of 16, padded to whole 32-key steps

// The kernel form of an attention call, HD * 100 + NKB, or -1 for a shape launch_attention_bf16 refuses: the
// predicate of the launcher, of the callers' checks ahead of their first launch, and of the report hook.
static int attention_bf16_form(int L, int C, int heads) {
  if (heads <= 0 || C <= 0 || C % heads != 0 || C % 8 != 0 || L <= 0 || L > 320) return -1;
  const int hd = C / heads, nkb = wattn_key_blocks(L);
  const int n = hd == 32 ? wattn_instance<32>(nkb) : hd == 64 ? wattn_instance<64>(nkb)
              : hd == 128 ? wattn_instance<128>(nkb) : -1;
  return n < 0 ? -1 : hd * 100 + n;
}
static int g_attn_bf16_last_form = -1;  // written where the launch happens, from the instance's own constants

template <int HD>
static int launch_wattn_hd(int nkb, dim3 grid, hipStream_t st, const bf16_t* qkv, int C, bf16_t* out,
                           const TokMap& tm, float scale) {
  const int inst = wattn_instance<HD>(nkb);
#define YS_WATTN(N)                                                                                             \
  if constexpr (wattn_lds_bytes<HD, N>() <= 160 * 1024) {                                                       \
    if (inst == N) {                                                                                            \
      hipLaunchKernelGGL((window_attn_bf16_kernel<HD, N>), grid, dim3(256), 0, st, qkv, C, out, tm, scale);     \
      g_attn_bf16_last_form = HD * 100 + N;                                                                     \
      return 0;                                                                                                 \
    }                                                                                                           \
  }
  YS_WATTN_ALL
#undef YS_WATTN
  YS_CHECK_ARG(false, "attention_bf16: %d key blocks of head dim %d unsupported", nkb, HD);
  return -1;
}
#undef YS_WATTN_ALL

static int launch_attention_bf16(const bf16_t* qkv, bf16_t* out, long n_seq, int C, int heads, const TokMap& tm,
                                 hipStream_t st) {
  YS_CHECK_ARG(heads > 0 && C % heads == 0, "attention_bf16: C=%d not divisible by heads=%d", C, heads);
  const int hd = C / heads;
  const int L = tm.L;
  YS_CHECK_ARG(L > 0 && L <= 320, "attention_bf16: sequence length %d unsupported (1..320)", L);
  YS_CHECK_ARG(n_seq < 65536, "attention_bf16: too many sequences (%ld)", n_seq);
  YS_CHECK_ARG(C % 8 == 0, "attention_bf16: C=%d must be a multiple of 8", C);
  YS_CHECK_ARG(hd == 32 || hd == 64 || hd == 128, "attention_bf16: head dim %d unsupported (32, 64, 128)", hd);
  YS_CHECK_ARG(attention_bf16_form(L, C, heads) >= 0,
               "attention_bf16: sequence length %d with head dim %d unsupported (no instance fits LDS)", L, hd);
  const int nkb = wattn_key_blocks(L);
  const float scale = 1.0f / sqrtf((float)hd);
  dim3 grid((L + 63) / 64, heads, (unsigned)n_seq);
  int rc;
  switch (hd) {
    case 32: rc = launch_wattn_hd<32>(nkb, grid, st, qkv, C, out, tm, scale); break;
    case 64: rc = launch_wattn_hd<64>(nkb, grid, st, qkv, C, out, tm, scale); break;
    case 128: rc = launch_wattn_hd<128>(nkb, grid, st, qkv, C, out, tm, scale); break;
    default: YS_CHECK_ARG(false, "attention_bf16: head dim %d unsupported (32, 64, 128)", hd);
  }
  if (rc) return rc;
  YS_CHECK_LAUNCH("attention_bf16");
  return 0;
}

// =================================================================================================
// Swin: depthwise 3x3 (pad 1, no bias) + bottom/right zero pad -> T[(img*Hp + h)*Wp + w][C] (padded raster order).
// grid = (B*Hp, ceil(C/64)): one padded row of one image and a 64-channel slab. Lane (c = tid/4, q = tid%4) computes
// runs of 8 pixels (q, q+4, ...) of channel c from three 16-byte row loads (+ the two neighbour pixels), so the input
// rows are read along w; the 8 results go to an LDS tile [w][64] and leave as 16-byte stores of 8 channels, so the
// token rows are written along c. Zero tokens for h >= H and w >= W (the reference pads after the conv).
// =================================================================================================
__global__ __launch_bounds__(256) void swin_tokens_bf16_kernel(const bf16_t* __restrict__ x,
                                                               const float* __restrict__ dw, bf16_t* __restrict__ T,
                                                               int C, int H, int W, int Hp, int Wp) {
  extern __shared__ __attribute__((aligned(16))) bf16_t tile[];  // [Wp][72]
  constexpr int TS = 72;
  const int img = blockIdx.x / Hp, h = blockIdx.x - (blockIdx.x / Hp) * Hp;
  const int c0 = blockIdx.y * 64;
  const int tid = threadIdx.x;
  bf16_t* Tr = T + ((long)img * Hp + h) * Wp * C + c0;
  if (h < H) {
    const int c = tid >> 2, q = tid & 3;
    const bool cok = c0 + c < C;
    const bf16_t* xc = x + ((long)img * C + c0 + (cok ? c : 0)) * H * W;
    float k[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) k[i] = cok ? dw[(long)(c0 + c) * 9 + i] : 0.f;
    const int nruns = (W + 7) >> 3;
    for (int run = q; run < nruns; run += 4) {
      const int w0 = run * 8;
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = 0.f;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int hh = h - 1 + r;
        if (hh < 0 || hh >= H || !cok) continue;
        const bf16_t* xr = xc + (long)hh * W;
        float v[10];
        v[0] = w0 > 0 ? bf2f(xr[w0 - 1]) : 0.f;
        if (w0 + 8 <= W && (W & 7) == 0) {
          float f[8];
          unpack8(*reinterpret_cast<const uint4*>(xr + w0), f);
#pragma unroll
          for (int j = 0; j < 8; ++j) v[1 + j] = f[j];
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[1 + j] = (w0 + j < W) ? bf2f(xr[w0 + j]) : 0.f;
        }
        v[9] = (w0 + 8 < W) ? bf2f(xr[w0 + 8]) : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] += k[3 * r] * v[j] + k[3 * r + 1] * v[j + 1] + k[3 * r + 2] * v[j + 2];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (w0 + j < Wp) tile[(w0 + j) * TS + c] = (w0 + j < W) ? f2bf(o[j]) : (bf16_t)0;
    }
    if (tid < 64)
      for (int w = ((W + 7) >> 3) * 8; w < Wp; ++w) tile[w * TS + tid] = 0;  // padding columns past the last run
  }
  __syncthreads();
  const int nc8 = ((C - c0 < 64) ? C - c0 : 64) >> 3;
  for (int e = tid; e < Wp * nc8; e += 256) {
    const int w = e / nc8, cc = e - (e / nc8) * nc8;
    const uint4 v = (h < H) ? *reinterpret_cast<const uint4*>(&tile[w * TS + 8 * cc]) : make_uint4(0u, 0u, 0u, 0u);
    *reinterpret_cast<uint4*>(Tr + (long)w * C + 8 * cc) = v;
  }
}

// Swin tokens + LN1 in one pass (W % 8 == 0, W <= 64, C % 64 == 0, C <= 1024): workgroup = one padded row of one
// image with all C channels. Thread c (then c + 256, ...) computes its channel's depthwise 3x3 over the whole row from
// three rows of W / 8 16-byte loads (the neighbour pixels come from the adjacent runs: no 2-byte loads), with the same
// expression and order as swin_tokens_bf16_kernel, into an LDS tile [Wp][C + 8]; then wave w normalises tokens w,
// w + 4, ... exactly as ln_rows_bf16_kernel (same lane -> channel map and sum order) and writes both the T row and the
// U = LN1(T) row. Bit-identical to swin_tokens_bf16_kernel + ln_rows_bf16_kernel; one launch and one HBM round trip
// of T less. dynamic LDS = Wp * (C + 8) * 2 bytes.
template <int VPL>
__global__ __launch_bounds__(256) void swin_tokens_ln_bf16_kernel(const bf16_t* __restrict__ x,
                                                                  const float* __restrict__ dw, bf16_t* __restrict__ T,
                                                                  bf16_t* __restrict__ U, int C, int H, int W, int Hp,
                                                                  int Wp, float eps, const float* __restrict__ lw,
                                                                  const float* __restrict__ lb) {
  extern __shared__ __attribute__((aligned(16))) bf16_t tile[];  // [Wp][C + 8]
  const int TS = C + 8;
  const int img = blockIdx.x / Hp, h = blockIdx.x - (blockIdx.x / Hp) * Hp;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nruns = W >> 3;
  for (int c = tid; c < C; c += 256) {
    if (h < H) {
      const bf16_t* xc = x + ((long)img * C + c) * H * W;
      float k[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) k[i] = dw[(long)c * 9 + i];
      uint4 rows[3][8];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int hh = h - 1 + r;
#pragma unroll
        for (int q = 0; q < 8; ++q)
          rows[r][q] = (q < nruns && hh >= 0 && hh < H) ? *reinterpret_cast<const uint4*>(xc + (long)hh * W + 8 * q)
                                                       : make_uint4(0u, 0u, 0u, 0u);
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        if (q >= nruns) break;
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = 0.f;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const int hh = h - 1 + r;
          if (hh < 0 || hh >= H) continue;
          float v[10], f[8];
          unpack8(rows[r][q], f);
          v[0] = 0.f;
          if (q > 0) {
            float pf[8];
            unpack8(rows[r][q - 1], pf);
            v[0] = pf[7];
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) v[1 + j] = f[j];
          v[9] = 0.f;
          if (q + 1 < nruns) {
            float nf[8];
            unpack8(rows[r][q + 1], nf);
            v[9] = nf[0];
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] += k[3 * r] * v[j] + k[3 * r + 1] * v[j + 1] + k[3 * r + 2] * v[j + 2];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) tile[(8 * q + j) * TS + c] = f2bf(o[j]);
      }
      for (int w = W; w < Wp; ++w) tile[w * TS + c] = (bf16_t)0;
    } else {
      for (int w = 0; w < Wp; ++w) tile[w * TS + c] = (bf16_t)0;
    }
  }
  __syncthreads();
  const int K4 = C >> 2;
  for (int w = wv; w < Wp; w += 4) {
    const long row = ((long)img * Hp + h) * Wp + w;
    const bf16_t* tr = tile + w * TS;
    f32x4 v[VPL];
    uint2 raw[VPL];
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < VPL; ++u) {
      const int c = lane + 64 * u;
      raw[u] = (c < K4) ? *reinterpret_cast<const uint2*>(tr + 4 * c) : make_uint2(0u, 0u);
      v[u] = f32x4{__uint_as_float(raw[u].x << 16), __uint_as_float(raw[u].x & 0xffff0000u),
                   __uint_as_float(raw[u].y << 16), __uint_as_float(raw[u].y & 0xffff0000u)};
      s += (v[u].x + v[u].y) + (v[u].z + v[u].w);
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int u = 0; u < VPL; ++u) {
      if (lane + 64 * u < K4) {
        const f32x4 d = v[u] - mean;
        q += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
      }
    }
    const float var = wave_sum(q) / (float)C;
    const float rs = 1.0f / sqrtf(var + eps);
#pragma unroll
    for (int u = 0; u < VPL; ++u) {
      const int c = lane + 64 * u;
      if (c < K4) {
        *reinterpret_cast<uint2*>(T + row * C + 4 * c) = raw[u];
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(lw + 4 * c), b4 = *reinterpret_cast<const f32x4*>(lb + 4 * c);
        f32x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = fmaf((v[u][i] - mean) * rs, w4[i], b4[i]);
        st4(U + row * C + 4 * c, o);
      }
    }
  }
}

// A2: adaptive-avg-pool over rows to A areas (overlapping bins), token-major S[(img*A + a)*W + w][c] (bf16).
__global__ __launch_bounds__(256) void a2_pool_tokens_bf16_kernel(const bf16_t* __restrict__ xp, bf16_t* __restrict__ S,
                                                                  int C, int H, int W, int A) {
  extern __shared__ float slab[];  // [64][W + 1]
  const int img = blockIdx.x / A, a = blockIdx.x % A;
  const int c0 = blockIdx.y * 64;
  const int nc = (C - c0 < 64) ? C - c0 : 64;
  const int r0 = (a * H) / A, r1 = ((a + 1) * H + A - 1) / A;
  const float inv = (float)(r1 - r0);
  const bf16_t* xb = xp + ((long)img * C + c0) * H * W;
  for (int e = threadIdx.x; e < nc * W; e += 256) {
    const int c = e / W, w = e - c * W;
    const bf16_t* src = xb + ((long)c * H + r0) * W + w;
    float s = 0.f;
    for (int r = 0; r < r1 - r0; ++r) s += bf2f(src[(long)r * W]);
    slab[c * (W + 1) + w] = s / inv;
  }
  __syncthreads();
  bf16_t* Sb = S + ((long)img * A + a) * W * C + c0;
  for (int e = threadIdx.x; e < nc * W; e += 256) {
    const int w = e / nc, c = e - w * nc;
    Sb[(long)w * C + c] = f2bf(slab[c * (W + 1) + w]);
  }
}

// A2 tail: y = x + SiLU(up_h(T) + b), T = out conv of the area tokens laid out [img][C][A][W] (bf16).
__global__ __launch_bounds__(256) void a2_upsample_out_bf16_kernel(const bf16_t* __restrict__ x,
                                                                   const bf16_t* __restrict__ T,
                                                                   const float* __restrict__ bias,
                                                                   bf16_t* __restrict__ y, int C, int H, int W,
                                                                   int A) {
  const long pc = blockIdx.x;  // img*C + c
  const int c = (int)(pc % C);
  const int e = blockIdx.y * 256 + threadIdx.x;
  if (e >= H * W) return;
  const int h = e / W, w = e - h * W;
  const float sc = (float)A / (float)H;
  float src = sc * ((float)h + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  const int y0 = (int)src;
  const int y1 = y0 + ((y0 < A - 1) ? 1 : 0);
  const float l1 = src - (float)y0, l0 = 1.0f - l1;
  const bf16_t* Tp = T + pc * A * W;
  const float u = l0 * bf2f(Tp[y0 * W + w]) + l1 * bf2f(Tp[y1 * W + w]);
  const long o = pc * H * W + e;
  y[o] = f2bf(bf2f(x[o]) + siluf_(u + bias[c]));
}

// The same tail with 4 consecutive elements of a plane per thread (H*W % 4 == 0): 8-byte x loads and y stores (the
// 2-byte form ran at ~1.3 TB/s). grid = ceil(planes * H*W / 1024); same arithmetic per element.
__global__ __launch_bounds__(256) void a2_upsample_out4_bf16_kernel(const bf16_t* __restrict__ x,
                                                                    const bf16_t* __restrict__ T,
                                                                    const float* __restrict__ bias,
                                                                    bf16_t* __restrict__ y, int C, int H, int W, int A,
                                                                    long total4) {
  const long i4 = (long)blockIdx.x * 256 + threadIdx.x;
  if (i4 >= total4) return;
  const long HW = (long)H * W;
  const long o = i4 * 4;
  const long pc = o / HW;  // img*C + c (HW % 4 == 0: the 4 elements share the plane)
  const int c = (int)(pc % C);
  const int e0 = (int)(o - pc * HW);
  const float sc = (float)A / (float)H;
  const bf16_t* Tp = T + pc * A * W;
  const float b = bias[c];
  const f32x4 xv = ld4(x + o);
  f32x4 r;
  // one division for the quad: its pixels are consecutive (a row change is a step of h)
  int h = e0 / W, w = e0 - h * W;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k > 0 && ++w == W) {
      w = 0;
      ++h;
    }
    float src = sc * ((float)h + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    const int y0 = (int)src;
    const int y1 = y0 + ((y0 < A - 1) ? 1 : 0);
    const float l1 = src - (float)y0, l0 = 1.0f - l1;
    const float u = l0 * bf2f(Tp[y0 * W + w]) + l1 * bf2f(Tp[y1 * W + w]);
    r[k] = xv[k] + silu_fast_(u + b);  // hardware exp2 / rcp (~2^-22 relative)
  }
  st4(y + o, r);
}

__global__ void fold_bn_bf16_kernel(const float* w, const float* b, const float* m, const float* v, float eps, int C,
                                    float* scale, float* shift) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const float inv = 1.0f / sqrtf(v[c] + eps);
  const float sc = w[c] * inv;
  scale[c] = sc;
  shift[c] = b[c] - m[c] * sc;
}

struct SwinGeomB {
  int wh, ww, Hp, Wp, nWx, nWin, L;
  long ntok;  // B * Hp * Wp
};
static SwinGeomB swin_geom_b(int B, int H, int W, int ws) {
  SwinGeomB g;
  g.wh = H < ws ? H : ws;
  g.ww = W < ws ? W : ws;
  if (H <= ws && W <= ws) {  // single global window, no pad (blocks_transformer.py:25-28)
    g.wh = H;
    g.ww = W;
  }
  g.Hp = H + (g.wh - H % g.wh) % g.wh;
  g.Wp = W + (g.ww - W % g.ww) % g.ww;
  g.nWx = g.Wp / g.ww;
  g.nWin = (g.Hp / g.wh) * g.nWx;
  g.L = g.wh * g.ww;
  g.ntok = (long)B * g.Hp * g.Wp;
  return g;
}

}  // namespace ys

using namespace ys;

bool yolosod_swin_fused_bf16_ok(int C, int num_heads, int wh, int ww, int mlp_hidden);
int yolosod_swin_fused_bf16_launch(const bf16_t* x, bf16_t* y, int B, int C, int H, int W, int num_heads, int wh,
                                   int ww, int nWx, int nWin, const float* dw_w, const float* ln1_w, const float* ln1_b,
                                   float ln1_eps, const bf16_t* in_proj_w, const float* in_proj_b,
                                   const bf16_t* out_proj_w, const float* out_proj_b, const float* ln2_w,
                                   const float* ln2_b, float ln2_eps, const bf16_t* mlp1_w, const float* mlp1_b,
                                   int mlp_hidden, const bf16_t* mlp2_w, const float* mlp2_b, const bf16_t* pw_w,
                                   const float* bn_scale, const float* bn_shift, bf16_t* wfrag, hipStream_t st);
size_t yolosod_swin_fused_bf16_wfrag_elems(int C, int mlp_hidden);
bool yolosod_swin_fused_bf16_takes(int B, int C, int num_heads, int wh, int ww, int nWin, int mlp_hidden);
bool yolosod_swin_fused_bf16_chunked(int W);
int yolosod_swin_fused_bf16_last_chunked(void);

// =================================================================================================
// C ABI (bf16 storage: activations / GEMM weights are bf16 bit patterns, other parameters fp32)
// =================================================================================================
YS_EXPORT int yolosod_gemm_bf16(const bf16_t* A, long a_bs, int lda, const bf16_t* B, long b_bs, int ldb,
                                int b_kcontig, bf16_t* C, long c_bs, int ldc, int M, int N, int K, int batch,
                                const float* bias, int bias_mode, int act, const bf16_t* res, void* stream) {
  GemmB g{};
  g.A = A; g.a_bs = a_bs; g.lda = lda;
  g.B = B; g.b_bs = b_bs; g.ldb = ldb;
  g.M = M; g.N = N; g.K = K;
  g.epi = epib_plain(C, c_bs, ldc);
  g.epi.bias = bias; g.epi.bias_mode = bias ? bias_mode : 0;
  g.epi.act = act;
  g.epi.res = res; g.epi.res_bs = c_bs; g.epi.ldr = ldc;
  return launch_gemm_bf16(g, batch, b_kcontig != 0, (hipStream_t)stream);
}

// Test hooks (host only, no launch). yolosod_debug_gemm_bf16_tile: the N extent of the tile launch_gemm_bf16 takes for
// (M, N, batch), 64 or 128, from the launcher's own rule. yolosod_debug_gemm_bf16_last_tile / _launches(tile): the tile
// of the last bf16 GEMM launch of this process (-1: none yet) and the launches with that tile so far, both written
// where the launch happens.
YS_EXPORT int yolosod_debug_gemm_bf16_tile(int M, int N, int batch) { return gemm_bf16_tile(M, N, batch); }
YS_EXPORT int yolosod_debug_gemm_bf16_last_tile(void) { return g_gemm_bf16_last_tile; }
YS_EXPORT long yolosod_debug_gemm_bf16_launches(int tile) {
  return tile == 64 ? g_gemm_bf16_launches[0] : tile == 128 ? g_gemm_bf16_launches[1] : -1;
}
// The attention kernel form for (L, C, heads): head dim * 100 + key blocks of the instance, -1 for a refused shape;
// and the form of the last attention launch of this process (-1: none yet).
YS_EXPORT int yolosod_debug_attention_bf16_form(int L, int C, int heads) { return attention_bf16_form(L, C, heads); }
YS_EXPORT int yolosod_debug_attention_bf16_last_form(void) { return g_attn_bf16_last_form; }

// Test hook: attention over contiguous sequences of L rows of a [n_seq*L][3C] bf16 QKV matrix -> [n_seq*L][C].
YS_EXPORT int yolosod_attention_bf16(const bf16_t* qkv, bf16_t* out, long n_seq, int L, int C, int heads,
                                     void* stream) {
  TokMap tm{};
  tm.mode = 0;
  tm.L = L;
  return launch_attention_bf16(qkv, out, n_seq, C, heads, tm, (hipStream_t)stream);
}

YS_EXPORT size_t yolosod_swin_workspace_bf16(int B, int C, int H, int W, int num_heads, int window, int mlp_hidden) {
  SwinGeomB g = swin_geom_b(B, H, W, window);
  if (yolosod_swin_fused_bf16_takes(B, C, num_heads, g.wh, g.ww, g.nWin, mlp_hidden)) {
    // fused per-window kernel: folded BN and the fragment-major weight copies
    Sizer s;
    s.take<float>((size_t)C * 2);
    s.take<bf16_t>(yolosod_swin_fused_bf16_wfrag_elems(C, mlp_hidden));
    return s.off;
  }
  const int wide = (3 * C > mlp_hidden) ? 3 * C : mlp_hidden;
  Sizer s;
  s.take<bf16_t>((size_t)g.ntok * C);     // T (residual stream)
  s.take<bf16_t>((size_t)g.ntok * C);     // U (attention out)
  s.take<bf16_t>((size_t)g.ntok * wide);  // QKV / MLP hidden
  s.take<float>((size_t)C * 2);           // folded BN
  s.take<float>((size_t)g.ntok * 2);      // LayerNorm row statistics
  return s.off;
}

// tokens + LN1 in one pass (swin_tokens_ln_bf16_kernel; the test hook selects the two-kernel form)
static int& tokens_ln_mode() {
  static int on = 1;
  return on;
}
static bool tokens_ln_env() { return tokens_ln_mode() != 0; }
YS_EXPORT int yolosod_debug_set_swin_tokln(int on) {
  const int prev = tokens_ln_mode();
  tokens_ln_mode() = on ? 1 : 0;
  return prev;
}
static size_t swin_tokln_lds(int C, int Wp) { return (size_t)Wp * (C + 8) * sizeof(bf16_t); }
static size_t swin_tok_lds(int Wp) { return (size_t)Wp * 72 * sizeof(bf16_t); }
// whether the decomposed path takes the tokens + LN1 pass (ln_aligned: ln1_w and ln1_b on 16 bytes)
static bool swin_tokln_takes(int C, int W, int Wp, bool ln_aligned) {
  return tokens_ln_env() && W % 8 == 0 && W <= 64 && C <= 1024 && swin_tokln_lds(C, Wp) <= 80 * 1024 && ln_aligned;
}

// Route report of the bf16 SwinBlock: 0 decomposed with the two-kernel token path, 1 decomposed with the tokens +
// LN1 pass, 2 fused per-window kernel with the 2-byte halo layout, 3 fused with the 16-byte chunk layout; -1 for a
// shape yolosod_swin_forward_bf16 refuses. The same predicates the forward calls, in its order.
enum { SWIN_BF16_TOK2 = 0, SWIN_BF16_TOKLN = 1, SWIN_BF16_FUSED_2B = 2, SWIN_BF16_FUSED_CHUNK = 3 };
static int g_swin_bf16_last_route = -1;  // written where the launches happen
static int swin_bf16_route(int B, int C, int heads, int H, int W, int window, int mlp_hidden, bool ln_aligned) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || window <= 0 || heads <= 0) return -1;
  if (C % 64 != 0 || mlp_hidden <= 0 || mlp_hidden % 64 != 0) return -1;
  const SwinGeomB g = swin_geom_b(B, H, W, window);
  if (g.L > 320 || g.ntok >= (1L << 31)) return -1;
  if (yolosod_swin_fused_bf16_takes(B, C, heads, g.wh, g.ww, g.nWin, mlp_hidden))
    return yolosod_swin_fused_bf16_chunked(W) ? SWIN_BF16_FUSED_CHUNK : SWIN_BF16_FUSED_2B;
  if (attention_bf16_form(g.L, C, heads) < 0 || (long)B * g.nWin >= 65536) return -1;
  if (swin_tokln_takes(C, W, g.Wp, ln_aligned)) return SWIN_BF16_TOKLN;
  return swin_tok_lds(g.Wp) <= 64 * 1024 ? SWIN_BF16_TOK2 : -1;
}
YS_EXPORT int yolosod_debug_swin_bf16_route(int B, int C, int num_heads, int H, int W, int window, int mlp_hidden) {
  return swin_bf16_route(B, C, num_heads, H, W, window, mlp_hidden, true);
}
// The route the last yolosod_swin_forward_bf16 call of this process took (-1: none yet).
YS_EXPORT int yolosod_debug_swin_bf16_last_route(void) { return g_swin_bf16_last_route; }

// SwinBlock.forward (blocks_transformer.py:150-171) on bf16 activations. Weights: in_proj [3C][C], out_proj [C][C],
// mlp1 [hid][C], mlp2 [C][hid], pw [C][C] bf16; dw [C][9], LN / biases / BN fp32.
YS_EXPORT int yolosod_swin_forward_bf16(const bf16_t* x, bf16_t* y, int B, int C, int H, int W, int num_heads,
                                        int window, const float* dw_w, const float* ln1_w, const float* ln1_b,
                                        float ln1_eps, const bf16_t* in_proj_w, const float* in_proj_b,
                                        const bf16_t* out_proj_w, const float* out_proj_b, const float* ln2_w,
                                        const float* ln2_b, float ln2_eps, const bf16_t* mlp1_w, const float* mlp1_b,
                                        int mlp_hidden, const bf16_t* mlp2_w, const float* mlp2_b,
                                        const bf16_t* pw_w, const float* bn_w, const float* bn_b,
                                        const float* bn_mean, const float* bn_var, float bn_eps, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  YS_CHECK_ARG(x && y && dw_w && ln1_w && ln1_b && in_proj_w && in_proj_b && out_proj_w && out_proj_b && ln2_w &&
                   ln2_b && mlp1_w && mlp1_b && mlp2_w && mlp2_b && pw_w && bn_w && bn_b && bn_mean && bn_var,
               "swin_bf16: null pointer");
  YS_CHECK_ARG(B >= 0 && C > 0 && H > 0 && W > 0 && window > 0 && num_heads > 0, "swin_bf16: bad shape");
  YS_CHECK_ARG(C % 64 == 0 && mlp_hidden % 64 == 0, "swin_bf16: C and mlp_hidden must be multiples of 64");
  if (B == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  SwinGeomB g = swin_geom_b(B, H, W, window);
  YS_CHECK_ARG(g.L <= 320, "swin_bf16: window of %d tokens unsupported", g.L);
  YS_CHECK_ARG(g.ntok < (1L << 31), "swin_bf16: too many tokens");
  if (yolosod_swin_fused_bf16_takes(B, C, num_heads, g.wh, g.ww, g.nWin, mlp_hidden)) {
    Carver cf(workspace, workspace_bytes);
    float* fold = cf.take<float>((size_t)C * 2);
    bf16_t* wfrag = cf.take<bf16_t>(yolosod_swin_fused_bf16_wfrag_elems(C, mlp_hidden));
    YS_CHECK_ARG(fold && wfrag, "swin_bf16: workspace too small (%zu)", workspace_bytes);
    hipLaunchKernelGGL(fold_bn_bf16_kernel, dim3((C + 255) / 256), dim3(256), 0, st, bn_w, bn_b, bn_mean, bn_var,
                       bn_eps, C, fold, fold + C);
    const int r = yolosod_swin_fused_bf16_launch(x, y, B, C, H, W, num_heads, g.wh, g.ww, g.nWx, g.nWin, dw_w, ln1_w,
                                                 ln1_b, ln1_eps, in_proj_w, in_proj_b, out_proj_w, out_proj_b, ln2_w,
                                                 ln2_b, ln2_eps, mlp1_w, mlp1_b, mlp_hidden, mlp2_w, mlp2_b, pw_w, fold,
                                                 fold + C, wfrag, st);
    if (r < 0) return -1;
    if (r == 1) {
      g_swin_bf16_last_route = yolosod_swin_fused_bf16_last_chunked() ? SWIN_BF16_FUSED_CHUNK : SWIN_BF16_FUSED_2B;
      return 0;
    }
  }
  // the attention's own refusals, ahead of the first launch
  YS_CHECK_ARG(attention_bf16_form(g.L, C, num_heads) >= 0,
               "swin_bf16: window of %d tokens with head dim %d/%d unsupported", g.L, C, num_heads);
  YS_CHECK_ARG((long)B * g.nWin < 65536, "swin_bf16: too many windows (%ld)", (long)B * g.nWin);
  Carver cv(workspace, workspace_bytes);
  bf16_t* T = cv.take<bf16_t>((size_t)g.ntok * C);
  bf16_t* U = cv.take<bf16_t>((size_t)g.ntok * C);
  const int wide = (3 * C > mlp_hidden) ? 3 * C : mlp_hidden;
  bf16_t* Q = cv.take<bf16_t>((size_t)g.ntok * wide);
  float* bn_fold = cv.take<float>((size_t)C * 2);
  float* lns = cv.take<float>((size_t)g.ntok * 2);
  YS_CHECK_ARG(lns, "swin_bf16: workspace too small (%zu)", workspace_bytes);
  int rc;
  // dwconv + pad -> T (raster tokens), and U = LN1(T) (U is free until the attention writes it)
  const size_t tokln_lds = swin_tokln_lds(C, g.Wp);
  if (swin_tokln_takes(C, W, g.Wp, ((uintptr_t)ln1_w | (uintptr_t)ln1_b) % 16 == 0)) {
    const dim3 grid((unsigned)(B * g.Hp));
    if (C <= 256)
      hipLaunchKernelGGL((swin_tokens_ln_bf16_kernel<1>), grid, dim3(256), tokln_lds, st, x, dw_w, T, U, C, H, W,
                         g.Hp, g.Wp, ln1_eps, ln1_w, ln1_b);
    else if (C <= 512)
      hipLaunchKernelGGL((swin_tokens_ln_bf16_kernel<2>), grid, dim3(256), tokln_lds, st, x, dw_w, T, U, C, H, W,
                         g.Hp, g.Wp, ln1_eps, ln1_w, ln1_b);
    else
      hipLaunchKernelGGL((swin_tokens_ln_bf16_kernel<4>), grid, dim3(256), tokln_lds, st, x, dw_w, T, U, C, H, W,
                         g.Hp, g.Wp, ln1_eps, ln1_w, ln1_b);
    YS_CHECK_LAUNCH("swin_tokens_ln_bf16");
    g_swin_bf16_last_route = SWIN_BF16_TOKLN;
  } else {
    const size_t tok_lds = swin_tok_lds(g.Wp);
    YS_CHECK_ARG(tok_lds <= 64 * 1024, "swin_bf16: W=%d too wide for the token kernel", W);
    hipLaunchKernelGGL(swin_tokens_bf16_kernel, dim3((unsigned)(B * g.Hp), (unsigned)((C + 63) / 64)), dim3(256),
                       tok_lds, st, x, dw_w, T, C, H, W, g.Hp, g.Wp);
    YS_CHECK_LAUNCH("swin_tokens_bf16");
    g_swin_bf16_last_route = SWIN_BF16_TOK2;
    // QKV = LN1(T) Win^T + b_in (LN1(T) -> U once, U is free until the attention writes it)
    if ((rc = launch_ln_rows_bf16(T, C, g.ntok, C, ln1_eps, ln1_w, ln1_b, U, C, st))) return rc;
  }
  GemmB ga{};
  ga.A = U; ga.lda = C; ga.B = in_proj_w; ga.ldb = C; ga.M = (int)g.ntok; ga.N = 3 * C; ga.K = C;
  ga.epi = epib_plain(Q, 0, 3 * C);
  ga.epi.bias = in_proj_b; ga.epi.bias_mode = 2;
  if ((rc = launch_gemm_bf16(ga, 1, true, st))) return rc;
  TokMap tm{};
  tm.mode = 1; tm.L = g.L; tm.Hp = g.Hp; tm.Wp = g.Wp; tm.wh = g.wh; tm.ww = g.ww; tm.nWx = g.nWx; tm.nWin = g.nWin;
  if ((rc = launch_attention_bf16(Q, U, (long)B * g.nWin, C, num_heads, tm, st))) return rc;
  // T = T + (O Wo^T + bo)
  ga = GemmB{};
  ga.A = U; ga.lda = C; ga.B = out_proj_w; ga.ldb = C; ga.M = (int)g.ntok; ga.N = C; ga.K = C;
  ga.epi = epib_plain(T, 0, C);
  ga.epi.bias = out_proj_b; ga.epi.bias_mode = 2; ga.epi.res = T; ga.epi.ldr = C;
  if ((rc = launch_gemm_bf16(ga, 1, true, st))) return rc;
  // Hd = GELU(LN2(T) W1^T + b1) (LN2(T) -> U: the out-projection has read it)
  if ((rc = launch_ln_rows_bf16(T, C, g.ntok, C, ln2_eps, ln2_w, ln2_b, U, C, st))) return rc;
  ga = GemmB{};
  ga.A = U; ga.lda = C; ga.B = mlp1_w; ga.ldb = C; ga.M = (int)g.ntok; ga.N = mlp_hidden; ga.K = C;
  ga.epi = epib_plain(Q, 0, mlp_hidden);
  ga.epi.bias = mlp1_b; ga.epi.bias_mode = 2; ga.epi.act = 2;
  if ((rc = launch_gemm_bf16(ga, 1, true, st))) return rc;
  // T = T + (Hd W2^T + b2)
  ga = GemmB{};
  ga.A = Q; ga.lda = mlp_hidden; ga.B = mlp2_w; ga.ldb = mlp_hidden; ga.M = (int)g.ntok; ga.N = C; ga.K = mlp_hidden;
  ga.epi = epib_plain(T, 0, C);
  ga.epi.bias = mlp2_b; ga.epi.bias_mode = 2; ga.epi.res = T; ga.epi.ldr = C;
  if ((rc = launch_gemm_bf16(ga, 1, true, st))) return rc;
  // y = x + SiLU(BN(pw . T)), tokens -> NCHW pixels with the crop: M = out channel, N = raster token
  float* bn_scale = bn_fold;
  float* bn_shift = bn_fold + C;
  hipLaunchKernelGGL(fold_bn_bf16_kernel, dim3((C + 255) / 256), dim3(256), 0, st, bn_w, bn_b, bn_mean, bn_var, bn_eps,
                     C, bn_scale, bn_shift);
  ga = GemmB{};
  ga.A = pw_w; ga.lda = C; ga.B = T; ga.ldb = C; ga.M = C; ga.N = (int)g.ntok; ga.K = C;
  ga.epi = epib_plain(y, 0, C);
  ga.epi.scale = bn_scale; ga.epi.shift = bn_shift; ga.epi.bn_mode = 1; ga.epi.act = 1;
  ga.epi.res = x;
  ga.epi.swin = 1; ga.epi.sw_H = H; ga.epi.sw_W = W; ga.epi.sw_Hp = g.Hp; ga.epi.sw_Wp = g.Wp;
  if ((rc = launch_gemm_bf16(ga, 1, true, st))) return rc;
  return 0;
}

YS_EXPORT size_t yolosod_a2_workspace_bf16(int B, int C, int H, int W, int num_areas) {
  const long ntok = (long)B * num_areas * W;
  Sizer s;
  s.take<bf16_t>((size_t)B * C * H * W);  // proj output
  s.take<bf16_t>((size_t)ntok * C);       // S / T
  s.take<bf16_t>((size_t)ntok * C);       // U
  s.take<bf16_t>((size_t)ntok * 3 * C);   // QKV
  s.take<float>((size_t)ntok * 2);        // LayerNorm row statistics
  return s.off;
}

// A2_Attn.forward (a2_attn.py:35-69) on bf16 activations, residual form, with the MHA out-projection folded into
// the output conv (oproj_w = Wconv . Wmha, oproj_b = Wconv . bmha + bconv; A2_Attn._fused_out). Weights proj
// [C][C], in_proj [3C][C], oproj [C][C] bf16; biases / LN fp32.
YS_EXPORT int yolosod_a2_forward_bf16(const bf16_t* x, bf16_t* y, int B, int C, int H, int W, int num_areas,
                                      int num_heads, const bf16_t* proj_w, const float* proj_b, const float* ln_w,
                                      const float* ln_b, float ln_eps, const bf16_t* in_proj_w,
                                      const float* in_proj_b, const bf16_t* oproj_w, const float* oproj_b,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  YS_CHECK_ARG(x && y && proj_w && proj_b && ln_w && ln_b && in_proj_w && in_proj_b && oproj_w && oproj_b,
               "a2_bf16: null pointer");
  YS_CHECK_ARG(B >= 0 && C > 0 && H > 0 && W > 0 && num_areas > 0, "a2_bf16: bad shape");
  YS_CHECK_ARG(C % 64 == 0, "a2_bf16: C must be a multiple of 64");
  YS_CHECK_ARG(((long)H * W) % 8 == 0, "a2_bf16: H*W must be a multiple of 8");
  // the attention's and the pooling kernel's own refusals, ahead of the first launch
  YS_CHECK_ARG((long)num_areas * W <= 320 && attention_bf16_form(num_areas * W, C, num_heads) >= 0,
               "a2_bf16: sequence of %ld tokens with head dim %d/%d unsupported", (long)num_areas * W, C, num_heads);
  YS_CHECK_ARG(B < 65536, "a2_bf16: too many images (%d)", B);
  YS_CHECK_ARG((size_t)64 * (W + 1) * sizeof(float) <= 64 * 1024, "a2_bf16: W=%d too large for the pooling kernel", W);
  if (B == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int A = num_areas;
  const long HW = (long)H * W;
  const long ntok = (long)B * A * W;
  Carver cv(workspace, workspace_bytes);
  bf16_t* XP = cv.take<bf16_t>((size_t)B * C * HW);
  bf16_t* S = cv.take<bf16_t>((size_t)ntok * C);
  bf16_t* U = cv.take<bf16_t>((size_t)ntok * C);
  bf16_t* Q = cv.take<bf16_t>((size_t)ntok * 3 * C);
  float* lns = cv.take<float>((size_t)ntok * 2);
  YS_CHECK_ARG(lns, "a2_bf16: workspace too small (%zu)", workspace_bytes);
  int rc;
  // XP = SiLU(Wp x + bp): M = Cout, N = HW (N-contiguous B), batched over images
  GemmB ga{};
  ga.A = proj_w; ga.lda = C; ga.B = x; ga.b_bs = C * HW; ga.ldb = (int)HW; ga.M = C; ga.N = (int)HW; ga.K = C;
  ga.epi = epib_plain(XP, C * HW, (int)HW);
  ga.epi.bias = proj_b; ga.epi.bias_mode = 1; ga.epi.act = 1;
  if ((rc = launch_gemm_bf16(ga, B, false, st))) return rc;
  hipLaunchKernelGGL(a2_pool_tokens_bf16_kernel, dim3(B * A, (C + 63) / 64), dim3(256),
                     (size_t)64 * (W + 1) * sizeof(float), st, XP, S, C, H, W, A);
  YS_CHECK_LAUNCH("a2_pool_bf16");
  // LN(S) -> U once (U is free until the attention writes it), then the QKV GEMM without an A prologue
  if ((rc = launch_ln_rows_bf16(S, C, ntok, C, ln_eps, ln_w, ln_b, U, C, st))) return rc;
  ga = GemmB{};
  ga.A = U; ga.lda = C; ga.B = in_proj_w; ga.ldb = C; ga.M = (int)ntok; ga.N = 3 * C; ga.K = C;
  ga.epi = epib_plain(Q, 0, 3 * C);
  ga.epi.bias = in_proj_b; ga.epi.bias_mode = 2;
  if ((rc = launch_gemm_bf16(ga, 1, true, st))) return rc;
  TokMap tm{};
  tm.mode = 0;
  tm.L = A * W;
  if ((rc = launch_attention_bf16(Q, U, B, C, num_heads, tm, st))) return rc;
  // T[img][n][t] = sum_c Wf[n][c] U[img*AW + t][c]   (S reused as T)
  bf16_t* T = S;
  ga = GemmB{};
  ga.A = oproj_w; ga.lda = C; ga.B = U; ga.b_bs = (long)A * W * C; ga.ldb = C; ga.M = C; ga.N = A * W; ga.K = C;
  ga.epi = epib_plain(T, (long)C * A * W, A * W);
  if ((rc = launch_gemm_bf16(ga, B, true, st))) return rc;
  if (HW % 4 == 0 && ((uintptr_t)x & 7) == 0 && ((uintptr_t)y & 7) == 0) {
    const long total4 = (long)B * C * HW / 4;
    hipLaunchKernelGGL(a2_upsample_out4_bf16_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, x, T,
                       oproj_b, y, C, H, W, A, total4);
  } else {
    hipLaunchKernelGGL(a2_upsample_out_bf16_kernel, dim3((unsigned)(B * C), (unsigned)((HW + 255) / 256)), dim3(256), 0,
                       st, x, T, oproj_b, y, C, H, W, A);
  }
  YS_CHECK_LAUNCH("a2_upsample_bf16");
  return 0;
}
