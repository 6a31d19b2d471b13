// ByteTrack on the device: track ids per video stream from the padded NMS rows, no host sync.
// The steps are the reference's BYTETracker.update (ultralytics/trackers/byte_tracker.py:293-405) as restated in
// yolo-sod_amd/utils/bytetrack.py, which is the definition this kernel is held to: frames[i] of every call is the next
// frame of stream i, a stream's update is sequential, streams are independent. One workgroup (256 lanes) per stream
// runs the whole update from device-resident state in one launch; no workgroup reads what another wrote.
//
// State, per stream, SoA over T slots (yolosod_track_state_bytes): a 64-byte header (frame, next id, overflow), the
// fp64 means [8][T] and covariances [64][T], then int32 state / flags / id / start frame / last frame / idx and fp32
// score / cls, each [T]. state: 0 free, 1 Tracked, 2 Lost, 3 Removed but still in the lost list (Q4: expiry is late by
// one frame). flags: bit 0 activated, bit 1 the id is in the reference's removed list (Q5).
//
// Phases, separated by workgroup barriers (every slot or detection is written by one lane between two barriers):
//   detections  fp32 boxes (xyxy for IoU as (l, t, l + w, t + h)), validity, tier (high / second)
//   predict     the pool (activated Tracked + Lost + Removed), one lane per track, fp64, closed block form of F P F'
//   associate 1 pool x high detections, fused scores, match_thresh; matched: Kalman update, state Tracked
//   associate 2 unmatched pool tracks whose state is Tracked x second tier, not fused, 0.5; unmatched: Lost
//   associate 3 unconfirmed x remaining high detections, fused, 0.7; unmatched: slot freed
//   births      remaining high detections with not (score < new_track_thresh), ascending row, lowest free slots
//   expiry      old lost tracks: Removed when frame - last > max_time_lost; dropped when already in the removed set
//   duplicates  (Tracked, lost) pairs with 1 - IoU < 0.15: the longer-lived side survives, ties drop the Tracked one
//   output      activated Tracked tracks, ascending id: (x1, y1, x2, y2, id, score, cls, idx)
//
// Costs are fp32 and bit-equal to the restatement (this file is built with -ffp-contract=off; IEEE division): the
// association's matrix is filled once by all lanes into the workspace ([n_tracks][n_dets] fp32 per stream, with the
// boxes next to it) and the solver reads one row per step, coalesced. T x D fp32 does not fit the LDS at T = 256,
// D = 300 beside the solver's arrays; at <= 300 KB per stream it stays in the XCD's L2, and a fill by 256 lanes is
// cheaper than recomputing an IoU (a division) every time the solver revisits a row.
//
// Assignment: the exact optimum of sum over matched (c_ij - thresh), which is what lapjv(extend_cost=True,
// cost_limit=thresh) solves. Rows are inserted one at a time by a shortest augmenting path (the Hungarian method in
// its dual-update form, fp64 duals) over the real columns with c_ij < thresh plus one private zero-cost "unmatched"
// column per row. A private column can only end a path: it is free whenever its row is in the tree, its dual stays 0,
// so only the cheapest one reached so far is kept, in registers. The column scan and the argmin run across the lanes.
// Every loop has a static bound from T and D, stated at the loop; none depends on floating-point convergence.
//
// BoT-SORT (the definition is yolo-sod_amd/utils/botsort.py) is the second instantiation of the same
// kernel, MODEL 1: the XYWH filter (kalman_filter.py:289-491: noise from the width and the height separately, state
// (cx, cy, w, h) and its velocities), both size velocities zeroed for tracks that are not Tracked (bot_sort.py:126-129),
// track boxes from (cx, cy, w, h) (bot_sort.py:110-117), and one more phase between predict and the first association:
//   gmc         every pool and unconfirmed track warped by the stream's 2x3 camera-motion matrix (STrack.multi_gmc,
//               byte_tracker.py:103-120), one lane per track, fp64, as the 2x2 blocks of kron(I4, R); a warp with a
//               non-finite entry is skipped and counted in the header (bad_warp)
// MODEL 0 is ByteTrack as before: it has no gmc phase and never touches the fourth header word.
#include "common.h"

namespace ys {
namespace trk {

constexpr int NT = 256;     // lanes per workgroup
constexpr int MAXN = 1024;  // largest T and D: NT lanes x 4 items in the compactions
static_assert(NT * 4 >= MAXN, "compact() gives every lane four items");
constexpr int ST_FREE = 0, ST_TRACKED = 1, ST_LOST = 2, ST_REMOVED = 3;
constexpr int FL_ACT = 1, FL_WASREM = 2;
constexpr int TI_POOL = 1, TI_OLDLOST = 2, TI_MATCHED = 4, TI_NEWLOST = 8, TI_UNCONF = 16;
constexpr int HDR_BYTES = 64;
constexpr int HDR_FRAME = 0, HDR_NEXT_ID = 1, HDR_OVERFLOW = 2, HDR_BAD_WARP = 3;
constexpr int XYAH = 0, XYWH = 1;  // the filter's model: ByteTrack, BoT-SORT
constexpr double STD_POS = 1.0 / 20, STD_VEL = 1.0 / 160;  // kalman_filter.py:62-63

__host__ __device__ inline size_t state_bytes(int T) { return HDR_BYTES + (size_t)T * (72 * 8 + 8 * 4); }
__host__ __device__ inline size_t ws_stream_bytes(int T, int D) {
  return ((size_t)T * D * 4 + (size_t)T * 16 + (size_t)D * 16 + 255) & ~(size_t)255;
}

struct View {  // one stream's state
  int* hdr;
  double* mean;  // [8][T]
  double* cov;   // [64][T]
  int *state, *flags, *tid, *start, *last, *idx;
  float *score, *cls;
};
__device__ __forceinline__ View view(char* base, int T) {
  View v;
  v.hdr = (int*)base;
  v.mean = (double*)(base + HDR_BYTES);
  v.cov = v.mean + 8 * (size_t)T;
  v.state = (int*)(v.cov + 64 * (size_t)T);
  v.flags = v.state + T;
  v.tid = v.flags + T;
  v.start = v.tid + T;
  v.last = v.start + T;
  v.idx = v.last + T;
  v.score = (float*)(v.idx + T);
  v.cls = v.score + T;
  return v;
}

struct Params {
  float high, low, newt, match, second, unconf;
  int max_time_lost, fuse;
};

struct Sh {  // 59 KB of LDS
  double u[MAXN], v[MAXN], minv[MAXN];  // solver: row duals, column duals, slack of the unused columns
  int p[MAXN], way[MAXN], x[MAXN];      // column -> row, column -> previous column of the path, row -> column
  int rows[MAXN], cols[MAXN];           // the association's slots and detection rows, ascending
  int dmatch[MAXN];                     // detection row -> slot it matched, -1
  int tmp[MAXN];
  float dscore[MAXN];
  unsigned char used[MAXN], tier[MAXN], tinfo[MAXN];
  double redv[NT / 64];
  int redc[NT / 64], scan[NT / 64];
};

// exclusive prefix sum of v over the workgroup's lanes, and the total; called by every lane
__device__ __forceinline__ int block_scan_excl(int v, int* s_w, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {  // 6 steps
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();  // the previous scan's totals have been read
  if (lane == 63) s_w[w] = inc;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < NT / 64; ++k) {
    const int t = s_w[k];
    if (k < w) base += t;
    total += t;
  }
  return base + inc - v;
}

// out = the indices i in [0, n) with pred(i), ascending; returns their number. n <= MAXN: lane t owns [4t, 4t + 4).
template <class Pred>
__device__ __forceinline__ int compact(int n, int* out, int* s_w, Pred pred) {
  const int base = threadIdx.x * 4;
  bool f[4];
  int c = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f[k] = base + k < n && pred(base + k);
    c += f[k] ? 1 : 0;
  }
  int total;
  int off = block_scan_excl(c, s_w, total);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (f[k]) out[off++] = base + k;
  __syncthreads();
  return total;
}

// ---- boxes ----------------------------------------------------------------------------------------------------------
// a detection row -> xyxy for IoU, xyah measurement, validity: bytetrack.det_boxes, fp32, one rounding per operation
__device__ __forceinline__ bool det_geom(const float* r, float4& xyxy, float4& xyah) {
  const float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3], sc = r[4];
  const float cx = (x1 + x2) / 2.f, cy = (y1 + y2) / 2.f, w = x2 - x1, h = y2 - y1;
  const float left = cx - w / 2.f, top = cy - h / 2.f;
  xyxy = make_float4(left, top, left + w, top + h);
  const bool valid = isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2) && isfinite(sc) && w > 0.f && h > 0.f;
  xyah = make_float4(left + w / 2.f, top + h / 2.f, w / (valid ? h : 1.f), h);
  return valid;
}
// the filter's measurement of a detection row: xyah, or for XYWH (l + w / 2, t + h / 2, w, h) (bot_sort.py:140-144)
template <int MODEL>
__device__ __forceinline__ float4 det_meas(const float* r) {
  float4 xyxy, z;
  det_geom(r, xyxy, z);
  if (MODEL == XYWH) z.z = r[2] - r[0];
  return z;
}
// a track's xyxy from its fp64 mean, one cast: bytetrack.track_boxes / botsort.track_boxes_xywh
template <int MODEL>
__device__ __forceinline__ float4 track_box(const View& st, int T, int slot) {
  const double m0 = st.mean[slot], m1 = st.mean[T + slot], m2 = st.mean[2 * T + slot], m3 = st.mean[3 * T + slot];
  const double w = MODEL == XYWH ? m2 : m2 * m3, left = m0 - w / 2.0, top = m1 - m3 / 2.0;
  return make_float4((float)left, (float)top, (float)(w + left), (float)(m3 + top));
}
// 1 - IoU of track box a against box b: bytetrack.iou_cost
__device__ __forceinline__ float iou_cost(float4 a, float4 b) {
  const float iw = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.f);
  const float ih = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.f);
  const float inter = iw * ih;
  const float area2 = (b.z - b.x) * (b.w - b.y), area1 = (a.z - a.x) * (a.w - a.y);
  const float area = (area2 + area1) - inter;
  return 1.f - inter / (area + 1e-7f);
}

// ---- Kalman filter, XYAH or XYWH, fp64, one lane per track ---------------------------------------------------------
template <int MODEL>
__device__ void kf_initiate(const View& st, int T, int slot, float4 z) {
  double var[8];
  if (MODEL == XYWH) {  // kalman_filter.py:351-361: eight fp32 products, squared in fp32 (the list is all np.float32)
    const float pw = 0.1f * z.z, ph = 0.1f * z.w, vw = 0.0625f * z.z, vh = 0.0625f * z.w;
    const float v32[8] = {pw * pw, ph * ph, pw * pw, ph * ph, vw * vw, vh * vh, vw * vw, vh * vh};
#pragma unroll
    for (int i = 0; i < 8; ++i) var[i] = (double)v32[i];
  } else {
    const double p = (double)(0.1f * z.w), v = (double)(0.0625f * z.w);  // fp32 products, then promoted
    const double std[8] = {p, p, 1e-2, p, v, v, 1e-5, v};
#pragma unroll
    for (int i = 0; i < 8; ++i) var[i] = std[i] * std[i];
  }
  const double m[4] = {(double)z.x, (double)z.y, (double)z.z, (double)z.w};
#pragma unroll
  for (int i = 0; i < 8; ++i) st.mean[i * T + slot] = i < 4 ? m[i] : 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) st.cov[(i * 8 + j) * T + slot] = i == j ? var[i] : 0.0;
}

// mean' = F mean, P' = F P F' + Q with F = [[I, I], [0, I]]: rows, then columns, then the diagonal; no 8x8 products
template <int MODEL>
__device__ void kf_predict(const View& st, int T, int slot, bool zero_vh) {
  double m[8], P[64];
#pragma unroll
  for (int i = 0; i < 8; ++i) m[i] = st.mean[i * T + slot];
#pragma unroll
  for (int i = 0; i < 64; ++i) P[i] = st.cov[i * T + slot];
  if (zero_vh) m[7] = 0.0;
  if (MODEL == XYWH && zero_vh) m[6] = 0.0;  // bot_sort.py:126-129
  double q[8];
  if (MODEL == XYWH) {  // kalman_filter.py:448-460
    const double pw = STD_POS * m[2], ph = STD_POS * m[3], vw = STD_VEL * m[2], vh = STD_VEL * m[3];
    q[0] = pw * pw, q[1] = ph * ph, q[2] = pw * pw, q[3] = ph * ph;
    q[4] = vw * vw, q[5] = vh * vh, q[6] = vw * vw, q[7] = vh * vh;
  } else {
    const double sp = STD_POS * m[3], sv = STD_VEL * m[3];
    q[0] = sp * sp, q[1] = sp * sp, q[2] = 1e-2 * 1e-2, q[3] = sp * sp;
    q[4] = sv * sv, q[5] = sv * sv, q[6] = 1e-5 * 1e-5, q[7] = sv * sv;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) m[i] = m[i] + m[i + 4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) P[i * 8 + j] = P[i * 8 + j] + P[(i + 4) * 8 + j];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) P[i * 8 + j] = P[i * 8 + j] + P[i * 8 + j + 4];
#pragma unroll
  for (int i = 0; i < 8; ++i) P[i * 9] = P[i * 9] + q[i];
#pragma unroll
  for (int i = 0; i < 8; ++i) st.mean[i * T + slot] = m[i];
#pragma unroll
  for (int i = 0; i < 64; ++i) st.cov[i * T + slot] = P[i];
}

// project, 4x4 Cholesky solve (unrolled, lower triangle as scipy's cho_factor(lower=True)), mean and covariance update
template <int MODEL>
__device__ void kf_update(const View& st, int T, int slot, float4 z32) {
  double m[8], P[64];
#pragma unroll
  for (int i = 0; i < 8; ++i) m[i] = st.mean[i * T + slot];
#pragma unroll
  for (int i = 0; i < 64; ++i) P[i] = st.cov[i * T + slot];
  const double sp = STD_POS * m[3], spw = STD_POS * m[2];
  const double r[4] = {MODEL == XYWH ? spw * spw : sp * sp, sp * sp, MODEL == XYWH ? spw * spw : 1e-1 * 1e-1, sp * sp};
  double S[16];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) S[i * 4 + j] = P[i * 8 + j] + (i == j ? r[i] : 0.0);
  // S = L L', from the lower triangle
  const double l00 = sqrt(S[0]);
  const double l10 = S[4] / l00, l20 = S[8] / l00, l30 = S[12] / l00;
  const double l11 = sqrt(S[5] - l10 * l10);
  const double l21 = (S[9] - l20 * l10) / l11, l31 = (S[13] - l30 * l10) / l11;
  const double l22 = sqrt(S[10] - l20 * l20 - l21 * l21);
  const double l32 = (S[14] - l30 * l20 - l31 * l21) / l22;
  const double l33 = sqrt(S[15] - l30 * l30 - l31 * l31 - l32 * l32);
  double K[32];  // the gain [8][4]: row k solves S x = P[k][0:4]
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double y0 = P[k * 8] / l00;
    const double y1 = (P[k * 8 + 1] - l10 * y0) / l11;
    const double y2 = (P[k * 8 + 2] - l20 * y0 - l21 * y1) / l22;
    const double y3 = (P[k * 8 + 3] - l30 * y0 - l31 * y1 - l32 * y2) / l33;
    const double x3 = y3 / l33;
    const double x2 = (y2 - l32 * x3) / l22;
    const double x1 = (y1 - l21 * x2 - l31 * x3) / l11;
    const double x0 = (y0 - l10 * x1 - l20 * x2 - l30 * x3) / l00;
    K[k * 4] = x0, K[k * 4 + 1] = x1, K[k * 4 + 2] = x2, K[k * 4 + 3] = x3;
  }
  const double inn[4] = {(double)z32.x - m[0], (double)z32.y - m[1], (double)z32.z - m[2], (double)z32.w - m[3]};
#pragma unroll
  for (int k = 0; k < 8; ++k)
    st.mean[k * T + slot] = m[k] + (inn[0] * K[k * 4] + inn[1] * K[k * 4 + 1] + inn[2] * K[k * 4 + 2] + inn[3] * K[k * 4 + 3]);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    double ks[4];  // row k of K S
#pragma unroll
    for (int j = 0; j < 4; ++j)
      ks[j] = K[k * 4] * S[j] + K[k * 4 + 1] * S[4 + j] + K[k * 4 + 2] * S[8 + j] + K[k * 4 + 3] * S[12 + j];
#pragma unroll
    for (int l = 0; l < 8; ++l)
      st.cov[(k * 8 + l) * T + slot] =
          P[k * 8 + l] - (ks[0] * K[l * 4] + ks[1] * K[l * 4 + 1] + ks[2] * K[l * 4 + 2] + ks[3] * K[l * 4 + 3]);
  }
}

// ---- camera motion (STrack.multi_gmc, byte_tracker.py:103-120), fp64, one lane per track ----------------------------
// mean' = kron(I4, R) mean with the translation added to (cx, cy); P' = kron(I4, R) P kron(I4, R)': the sixteen 2x2
// blocks R C_ij R', each read, transformed and written in place. R = [[a, b], [c, d]], t = (tx, ty).
__device__ void gmc_apply(const View& st, int T, int slot, double a, double b, double tx, double c, double d,
                          double ty) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double x = st.mean[(2 * i) * T + slot], y = st.mean[(2 * i + 1) * T + slot];
    double nx = a * x + b * y, ny = c * x + d * y;
    if (i == 0) nx += tx, ny += ty;
    st.mean[(2 * i) * T + slot] = nx;
    st.mean[(2 * i + 1) * T + slot] = ny;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double* p = st.cov + ((size_t)(2 * i) * 8 + 2 * j) * T + slot;  // C_ij = [[p00, p01], [p10, p11]]
      const double p00 = p[0], p01 = p[T], p10 = p[8 * (size_t)T], p11 = p[9 * (size_t)T];
      const double m00 = a * p00 + b * p10, m01 = a * p01 + b * p11;  // R C_ij
      const double m10 = c * p00 + d * p10, m11 = c * p01 + d * p11;
      p[0] = m00 * a + m01 * b;  // (R C_ij) R'
      p[T] = m00 * c + m01 * d;
      p[8 * (size_t)T] = m10 * a + m11 * b;
      p[9 * (size_t)T] = m10 * c + m11 * d;
    }
}

// ---- one association --------------------------------------------------------------------------------------------------
// s.rows[0..n_r) slots and s.cols[0..n_c) detection rows, both ascending. Fills the cost matrix, solves the exact
// assignment, applies the matches (Kalman update, state) and gives every unmatched slot the state ``unmatched`` (-1:
// leave it). Called by every lane.
template <int MODEL>
__device__ void associate(Sh& s, const View& st, int T, int n_r, int n_c, float thresh, bool fused, float* cost,
                          float4* tbox, const float4* dbox, const float* det, int frame, int unmatched) {
  const int tid = threadIdx.x;
  for (int r = tid; r < n_r; r += NT) {  // <= T / NT passes
    s.x[r] = -1;
    s.u[r] = 0.0;
    if (n_c > 0) tbox[r] = track_box<MODEL>(st, T, s.rows[r]);
  }
  for (int c = tid; c < n_c; c += NT) {  // <= D / NT passes
    s.v[c] = 0.0;
    s.p[c] = -1;
  }
  __syncthreads();
  if (n_r > 0 && n_c > 0) {
    for (int e = tid; e < n_r * n_c; e += NT) {  // <= T * D / NT passes
      const int r = e / n_c, c = e - r * n_c;
      const int d = s.cols[c];
      float cst = iou_cost(tbox[r], dbox[d]);
      if (fused) cst = 1.f - (1.f - cst) * s.dscore[d];  // fuse_score, matching.py:153-157
      cost[e] = cst;
    }
    __syncthreads();
    const double inf = __builtin_huge_val();
    const double thr = (double)thresh;
    // rows are inserted one at a time: exactly n_r <= T augmentations
    for (int r0 = 0; r0 < n_r; ++r0) {
      for (int c = tid; c < n_c; c += NT) {  // <= D / NT passes
        s.minv[c] = inf;
        s.used[c] = 0;
      }
      __syncthreads();
      double dummy_min = inf;  // the cheapest private column reached so far, its row; uniform over the lanes
      int dummy_row = -1;
      int i = r0, j0 = -1, j1 = -1;
      int terminal = 0;  // 1: a free real column j1, 2: dummy_row's private column
      // every step that does not end the path puts one more matched column, with its distinct matched row, into the
      // tree; fewer than n_r rows are matched, so at most n_r steps
      for (int step = 0; step <= n_r && !terminal; ++step) {
        const double ui = s.u[i];
        if (-ui < dummy_min) dummy_min = -ui, dummy_row = i;
        double best = inf;
        int bestc = 0x7fffffff;
        const float* crow = cost + (size_t)i * n_c;
        for (int c = tid; c < n_c; c += NT) {  // <= D / NT passes
          if (s.used[c]) continue;
          const float cf = crow[c];
          double mv = s.minv[c];
          if (cf < thresh) {  // a pair with c - thresh >= 0 is never useful; a NaN cost is none either
            const double cur = (((double)cf - thr) - ui) - s.v[c];
            if (cur < mv) {
              mv = cur;
              s.minv[c] = cur;
              s.way[c] = j0;
            }
          }
          if (mv < best) best = mv, bestc = c;  // ascending c: the lowest column of equal minima
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {  // 6 steps
          const double ov = __shfl_xor(best, o, 64);
          const int oc = __shfl_xor(bestc, o, 64);
          if (ov < best || (ov == best && oc < bestc)) best = ov, bestc = oc;
        }
        if ((tid & 63) == 0) s.redv[tid >> 6] = best, s.redc[tid >> 6] = bestc;
        __syncthreads();
        best = s.redv[0], bestc = s.redc[0];
#pragma unroll
        for (int k = 1; k < NT / 64; ++k) {
          const double ov = s.redv[k];
          const int oc = s.redc[k];
          if (ov < best || (ov == best && oc < bestc)) best = ov, bestc = oc;
        }
        double delta;
        if (dummy_min <= best) {
          delta = dummy_min;
          terminal = 2;
        } else {
          delta = best;
          j1 = bestc;
        }
        for (int c = tid; c < n_c; c += NT) {  // <= D / NT passes
          if (s.used[c]) {
            s.u[s.p[c]] += delta;  // distinct used columns hold distinct rows
            s.v[c] -= delta;
          } else {
            s.minv[c] -= delta;
            if (terminal == 0 && c == j1) s.used[c] = 1;  // by the column's own lane: no other lane reads it here
          }
        }
        if (tid == 0) s.u[r0] += delta;  // the root row
        dummy_min -= delta;
        __syncthreads();
        if (terminal == 0) {
          const int pi = s.p[j1];
          if (pi < 0) {
            terminal = 1;
          } else {
            j0 = j1;
            i = pi;
          }
        }
      }
      if (tid == 0 && terminal != 0) {
        int j;
        if (terminal == 1) {
          j = j1;
        } else {
          j = dummy_row == r0 ? -1 : s.x[dummy_row];
          s.x[dummy_row] = -1;
        }
        // the path back to the root: one column per step, at most n_r columns are in the tree
        for (int it = 0; it <= n_r && j >= 0; ++it) {
          const int jp = s.way[j];
          const int row = jp < 0 ? r0 : s.p[jp];
          s.p[j] = row;
          s.x[row] = j;
          j = jp;
        }
      }
      __syncthreads();
    }
  }
  for (int r = tid; r < n_r; r += NT) {  // <= T / NT passes
    const int slot = s.rows[r], c = s.x[r];
    if (c >= 0) {
      const int d = s.cols[c];
      const float* row = det + (size_t)d * 6;
      // STrack.update / re_activate(new_id=False), byte_tracker.py:137-178
      kf_update<MODEL>(st, T, slot, det_meas<MODEL>(row));
      st.state[slot] = ST_TRACKED;
      st.flags[slot] |= FL_ACT;
      st.last[slot] = frame;
      st.score[slot] = row[4];
      st.cls[slot] = row[5];
      st.idx[slot] = d;
      s.dmatch[d] = slot;
      s.tinfo[slot] |= TI_MATCHED;
    } else if (unmatched >= 0) {
      st.state[slot] = unmatched;
      if (unmatched == ST_LOST) s.tinfo[slot] |= TI_NEWLOST;
    }
  }
  __syncthreads();
}

template <int MODEL>
__global__ __launch_bounds__(NT) void track_update_kernel(char* __restrict__ state, int T, const float* __restrict__ det_all,
                                                          const int* __restrict__ counts, int D, Params prm,
                                                          float* __restrict__ tracks, int* __restrict__ n_tracks,
                                                          char* __restrict__ workspace, const double* __restrict__ warps) {
  __shared__ Sh s;
  const int b = blockIdx.x, tid = threadIdx.x;
  const View st = view(state + (size_t)b * state_bytes(T), T);
  char* ws = workspace + (size_t)b * ws_stream_bytes(T, D);
  float4* tbox = (float4*)ws;   // [T]
  float4* dbox = tbox + T;      // [D]
  float* cost = (float*)(dbox + D);  // [T * D]
  const float* det = det_all + (size_t)b * D * 6;
  const int n = min(max(counts[b], 0), D);
  const int frame = st.hdr[HDR_FRAME] + 1;  // byte_tracker.py:295
  const int next_id0 = st.hdr[HDR_NEXT_ID], overflow0 = st.hdr[HDR_OVERFLOW], bad_warp0 = st.hdr[HDR_BAD_WARP];

  // detections (byte_tracker.py:301-317)
  for (int d = tid; d < n; d += NT) {  // <= D / NT passes
    float4 xyxy, xyah;
    const bool valid = det_geom(det + (size_t)d * 6, xyxy, xyah);
    const float sc = det[(size_t)d * 6 + 4];
    dbox[d] = xyxy;
    s.dscore[d] = sc;
    s.tier[d] = !valid ? 0 : (sc >= prm.high ? 1 : ((sc > prm.low && sc < prm.high) ? 2 : 0));
    s.dmatch[d] = -1;
  }
  // the pool and its prediction (byte_tracker.py:321-331)
  for (int t = tid; t < T; t += NT) {  // T / NT passes
    const int sv = st.state[t];
    const bool act = (st.flags[t] & FL_ACT) != 0;
    int ti = 0;
    if ((sv == ST_TRACKED && act) || sv == ST_LOST || sv == ST_REMOVED) {
      ti = TI_POOL | (sv != ST_TRACKED ? TI_OLDLOST : 0);
      kf_predict<MODEL>(st, T, t, sv != ST_TRACKED);
    } else if (sv == ST_TRACKED) {
      ti = TI_UNCONF;
    }
    s.tinfo[t] = (unsigned char)ti;
  }
  // camera motion (byte_tracker.py:332-335): the pool after its prediction and the unconfirmed tracks, which were not
  // predicted. The lane that owns slot t here owned it in the loop above, so no barrier lies between the two. The six
  // values and the finite check are the same for every lane of the workgroup.
  int bad_warp = 0;
  if (MODEL == XYWH && warps) {
    const double* h = warps + (size_t)b * 6;
    const double a = h[0], bb = h[1], tx = h[2], c = h[3], d = h[4], ty = h[5];
    if (isfinite(a) && isfinite(bb) && isfinite(tx) && isfinite(c) && isfinite(d) && isfinite(ty)) {
      for (int t = tid; t < T; t += NT)  // T / NT passes
        if (s.tinfo[t] & (TI_POOL | TI_UNCONF)) gmc_apply(st, T, t, a, bb, tx, c, d, ty);
    } else {
      bad_warp = 1;
    }
  }
  __syncthreads();

  // first association (byte_tracker.py:337-348)
  int n_r = compact(T, s.rows, s.scan, [&](int t) { return (s.tinfo[t] & TI_POOL) != 0; });
  int n_c = compact(n, s.cols, s.scan, [&](int d) { return s.tier[d] == 1; });
  associate<MODEL>(s, st, T, n_r, n_c, prm.match, prm.fuse != 0, cost, tbox, dbox, det, frame, -1);
  // second association (byte_tracker.py:350-369)
  n_r = compact(T, s.rows, s.scan, [&](int t) {
    return (s.tinfo[t] & (TI_POOL | TI_MATCHED)) == TI_POOL && st.state[t] == ST_TRACKED;
  });
  n_c = compact(n, s.cols, s.scan, [&](int d) { return s.tier[d] == 2; });
  associate<MODEL>(s, st, T, n_r, n_c, prm.second, false, cost, tbox, dbox, det, frame, ST_LOST);
  // unconfirmed tracks (byte_tracker.py:371-380)
  n_r = compact(T, s.rows, s.scan, [&](int t) { return (s.tinfo[t] & TI_UNCONF) != 0; });
  n_c = compact(n, s.cols, s.scan, [&](int d) { return s.tier[d] == 1 && s.dmatch[d] < 0; });
  associate<MODEL>(s, st, T, n_r, n_c, prm.unconf, prm.fuse != 0, cost, tbox, dbox, det, frame, ST_FREE);

  // births (byte_tracker.py:382-387): ascending row index into the lowest free slots
  const int n_free = compact(T, s.rows, s.scan, [&](int t) { return st.state[t] == ST_FREE; });
  const int n_want = compact(n, s.cols, s.scan, [&](int d) {
    return s.tier[d] == 1 && s.dmatch[d] < 0 && !(s.dscore[d] < prm.newt);
  });
  const int n_born = min(n_free, n_want);
  for (int k = tid; k < n_born; k += NT) {  // <= T / NT passes
    const int slot = s.rows[k], d = s.cols[k];
    const float* row = det + (size_t)d * 6;
    kf_initiate<MODEL>(st, T, slot, det_meas<MODEL>(row));
    st.state[slot] = ST_TRACKED;
    st.flags[slot] = frame == 1 ? FL_ACT : 0;  // byte_tracker.py:130-131
    st.tid[slot] = next_id0 + k;
    st.start[slot] = frame;
    st.last[slot] = frame;
    st.score[slot] = row[4];
    st.cls[slot] = row[5];
    st.idx[slot] = d;
    s.tinfo[slot] = 0;
  }
  __syncthreads();

  // expiry (byte_tracker.py:389-401)
  for (int t = tid; t < T; t += NT) {  // T / NT passes
    const int ti = s.tinfo[t];
    int fl = st.flags[t];
    if ((ti & (TI_OLDLOST | TI_MATCHED)) == TI_OLDLOST) {
      const bool pend = frame - st.last[t] > prm.max_time_lost;
      if (pend) st.state[t] = ST_REMOVED;
      if (fl & FL_WASREM) st.state[t] = ST_FREE;
      if (pend) st.flags[t] = fl | FL_WASREM;
    } else if ((ti & TI_NEWLOST) && (fl & FL_WASREM)) {
      st.state[t] = ST_FREE;
    }
    s.tmp[t] = 0;  // the duplicate marks
  }
  __syncthreads();

  // duplicates (byte_tracker.py:400, 464-476)
  const int n_a = compact(T, s.rows, s.scan, [&](int t) { return st.state[t] == ST_TRACKED; });
  const int n_b = compact(T, s.cols, s.scan, [&](int t) { return st.state[t] == ST_LOST || st.state[t] == ST_REMOVED; });
  if (n_a > 0 && n_b > 0) {
    for (int t = tid; t < T; t += NT)  // T / NT passes
      if (st.state[t] != ST_FREE) tbox[t] = track_box<MODEL>(st, T, t);
    __syncthreads();
    for (int e = tid; e < n_a * n_b; e += NT) {  // <= T * T / (4 NT) passes
      const int ia = e / n_b, ib = e - ia * n_b;
      const int sa = s.rows[ia], sb = s.cols[ib];
      if (iou_cost(tbox[sa], tbox[sb]) < 0.15f) {
        const int timep = st.last[sa] - st.start[sa], timeq = st.last[sb] - st.start[sb];
        s.tmp[timep > timeq ? sb : sa] = 1;  // every writer stores the same value
      }
    }
    __syncthreads();
    for (int t = tid; t < T; t += NT)  // T / NT passes
      if (s.tmp[t]) st.state[t] = ST_FREE;
    __syncthreads();
  }

  // output (byte_tracker.py:405), ascending id: a track's rank is the number of live tracks with a smaller id
  const int n_live = compact(T, s.rows, s.scan, [&](int t) { return st.state[t] == ST_TRACKED && (st.flags[t] & FL_ACT); });
  for (int k = tid; k < n_live; k += NT) s.cols[k] = st.tid[s.rows[k]];  // <= T / NT passes
  __syncthreads();
  float* out = tracks + (size_t)b * T * 8;
  for (int k = tid; k < T; k += NT) {  // T / NT passes
    if (k < n_live) {
      const int slot = s.rows[k], id = s.cols[k];
      int rank = 0;
      for (int q = 0; q < n_live; ++q) rank += s.cols[q] < id ? 1 : 0;  // <= T steps; ids are distinct
      const float4 box = track_box<MODEL>(st, T, slot);
      float* o = out + (size_t)rank * 8;
      o[0] = box.x, o[1] = box.y, o[2] = box.z, o[3] = box.w;
      o[4] = (float)id, o[5] = st.score[slot], o[6] = st.cls[slot], o[7] = (float)st.idx[slot];
    } else {
      float* o = out + (size_t)k * 8;  // ranks fill [0, n_live): rows k >= n_live are padding
#pragma unroll
      for (int q = 0; q < 8; ++q) o[q] = 0.f;
    }
  }
  if (tid == 0) {
    n_tracks[b] = n_live;
    st.hdr[HDR_FRAME] = frame;
    st.hdr[HDR_NEXT_ID] = next_id0 + n_born;
    st.hdr[HDR_OVERFLOW] = overflow0 + (n_want - n_born);
    if (MODEL == XYWH && bad_warp) st.hdr[HDR_BAD_WARP] = bad_warp0 + 1;
  }
}

// zero a stream's state and start its ids at 1; workgroup k resets stream streams[k] (or k with streams == NULL)
__global__ __launch_bounds__(NT) void track_reset_kernel(char* __restrict__ state, int B, int T,
                                                         const int* __restrict__ streams) {
  const int b = streams ? streams[blockIdx.x] : (int)blockIdx.x;
  if (b < 0 || b >= B) return;
  int* w = (int*)(state + (size_t)b * state_bytes(T));
  const int words = (int)(state_bytes(T) / 4);
  for (int i = threadIdx.x; i < words; i += NT) w[i] = i == HDR_NEXT_ID ? 1 : 0;  // words / NT passes
}

static thread_local int g_last[8] = {0, 0, 0, 0, 0, 0, 0, 0};

static int check_shape(const char* what, int B, int T) {
  YS_CHECK_ARG(B >= 1, "%s: B=%d", what, B);
  YS_CHECK_ARG(T >= 64 && T <= MAXN && T % 64 == 0, "%s: T=%d unsupported (a multiple of 64 in 64..%d)", what, T, MAXN);
  return 0;
}

}  // namespace trk
}  // namespace ys

using namespace ys;

YS_EXPORT size_t yolosod_track_state_bytes(int T) { return T > 0 ? trk::state_bytes(T) : 0; }

YS_EXPORT size_t yolosod_track_workspace(int B, int T, int D) {
  return (B > 0 && T > 0 && D > 0) ? (size_t)B * trk::ws_stream_bytes(T, D) : 0;
}

YS_EXPORT int yolosod_track_reset(void* state, int B, int T, const int* streams, int n, void* stream) {
  using namespace trk;
  YS_CHECK_ARG(state, "track_reset: null pointer");
  if (check_shape("track_reset", B, T)) return -1;
  YS_CHECK_ARG(((uintptr_t)state & 7) == 0 && ((uintptr_t)streams & 3) == 0, "track_reset: misaligned pointer");
  const int grid = streams ? n : B;
  YS_CHECK_ARG(grid >= 0 && grid <= B, "track_reset: n=%d streams listed for B=%d", n, B);
  if (grid == 0) return 0;
  hipLaunchKernelGGL(track_reset_kernel, dim3((unsigned)grid), dim3(NT), 0, (hipStream_t)stream, (char*)state, B, T,
                     streams);
  YS_CHECK_LAUNCH("track_reset");
  return 0;
}

namespace ys {
namespace trk {
// the checks and the launch of both entry points; ``what`` names the caller in the messages
static int launch_update(const char* what, void* state, int B, int T, const float* det, const int* counts, int D,
                         const float* params, int model, const double* warps, float* tracks, int* n_tracks,
                         void* workspace, size_t ws_bytes, void* stream) {
  YS_CHECK_ARG(state && det && counts && params && tracks && n_tracks && workspace, "%s: null pointer", what);
  if (check_shape(what, B, T)) return -1;
  YS_CHECK_ARG(D >= 1 && D <= MAXN, "%s: D=%d unsupported (1..%d)", what, D, MAXN);
  YS_CHECK_ARG(model == XYAH || model == XYWH, "%s: model=%d unknown (0 XYAH, 1 XYWH)", what, model);
  YS_CHECK_ARG(!(warps && model == XYAH), "%s: warps with model 0 (XYAH, ByteTrack has no camera-motion step)", what);
  YS_CHECK_ARG(ws_bytes >= (size_t)B * ws_stream_bytes(T, D), "%s: workspace of %zu bytes, %zu needed", what, ws_bytes,
               (size_t)B * ws_stream_bytes(T, D));
  YS_CHECK_ARG(((uintptr_t)state & 7) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)det & 3) == 0 &&
                   ((uintptr_t)counts & 3) == 0 && ((uintptr_t)tracks & 3) == 0 && ((uintptr_t)n_tracks & 3) == 0,
               "%s: misaligned pointer", what);
  YS_CHECK_ARG(((uintptr_t)warps & 7) == 0, "%s: misaligned warps (8-byte alignment expected)", what);
  for (int i = 0; i < 8; ++i)
    YS_CHECK_ARG(params[i] >= 0.f && params[i] <= 3.402823466e+38f, "%s: params[%d] is %g (finite and >= 0 expected)", what,
                 i, (double)params[i]);
  Params prm;
  prm.high = params[0], prm.low = params[1], prm.newt = params[2], prm.match = params[3], prm.second = params[4];
  prm.unconf = params[5];
  prm.max_time_lost = params[6] > 2147483000.f ? 2147483000 : (int)params[6];
  prm.fuse = params[7] != 0.f;
  if (model == XYWH)
    hipLaunchKernelGGL(track_update_kernel<XYWH>, dim3((unsigned)B), dim3(NT), 0, (hipStream_t)stream, (char*)state, T,
                       det, counts, D, prm, tracks, n_tracks, (char*)workspace, warps);
  else
    hipLaunchKernelGGL(track_update_kernel<XYAH>, dim3((unsigned)B), dim3(NT), 0, (hipStream_t)stream, (char*)state, T,
                       det, counts, D, prm, tracks, n_tracks, (char*)workspace, (const double*)nullptr);
  YS_CHECK_LAUNCH(what);
  g_last[0] = T, g_last[1] = D, g_last[2] = B, g_last[3] = 1, g_last[4] = NT, g_last[5] = (int)ws_stream_bytes(T, D);
  g_last[6] = model, g_last[7] = warps ? 1 : 0;
  return 0;
}
}  // namespace trk
}  // namespace ys

YS_EXPORT int yolosod_track_update(void* state, int B, int T, const float* det, const int* counts, int D,
                                   const float* params, float* tracks, int* n_tracks, void* workspace, size_t ws_bytes,
                                   void* stream) {
  return trk::launch_update("track_update", state, B, T, det, counts, D, params, trk::XYAH, nullptr, tracks, n_tracks,
                            workspace, ws_bytes, stream);
}

YS_EXPORT int yolosod_track_update_ex(void* state, int B, int T, const float* det, const int* counts, int D,
                                      const float* params, int model, const double* warps, float* tracks, int* n_tracks,
                                      void* workspace, size_t ws_bytes, void* stream) {
  return trk::launch_update("track_update_ex", state, B, T, det, counts, D, params, model, warps, tracks, n_tracks,
                            workspace, ws_bytes, stream);
}

// host-side facts of this thread's last track_update launch: 0 T, 1 D, 2 B, 3 the workspace layout (1: per stream
// track boxes [T], detection boxes [D], cost matrix [T x D] fp32), 4 lanes per workgroup, 5 workspace bytes per stream,
// 6 the model (0 XYAH, 1 XYWH), 7 whether warps were given
YS_EXPORT int yolosod_debug_track_last(int what) { return (what >= 0 && what < 8) ? trk::g_last[what] : -1; }
