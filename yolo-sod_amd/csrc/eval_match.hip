// Validation, the step between NMS and the AP arithmetic: which detections are true positives at which IoU threshold
// (ultralytics/engine/validator.py:222-262 match_predictions, greedy path, over ultralytics/utils/metrics.py:52-71
// box_iou), for a whole batch of padded NMS rows in one launch and without a host sync.
//
// The reference works threshold by threshold (nonzero, argsort, two np.unique). Its result for one image with labels
// l = 0..L-1 and detections d = 0..n-1 in NMS order is exactly (tests/eval_match_ref.py):
//   iou[l][d]  box_iou in fp32, one rounding per operation, no FMA contraction (this file is built with
//              -ffp-contract=off), IEEE division:  w = max(min(x2) - max(x1), 0), h likewise, inter = w * h,
//              iou = inter / (((a_l + a_d) - inter) + 1e-7f);  0 where the classes differ (compared as fp32)
//   bi[d]      max_l iou[l][d];  best[d] the label that attains it, the highest index on a tie, none if bi[d] == 0
//   m[d]       max{ bi[d'] : d' < d, best[d'] == best[d] }, 0 if there is no such d'
//   tp[d][t]   bi[d] >= thr_t and thr_t > m[d]                      (thr_t > 0)
// The best label does not depend on the threshold, so one pass over the labels serves all thresholds.
//
// One workgroup per image, one lane per detection row (D <= 1024 rows, the block is D rounded up to whole waves).
// counts[b], label_off[b] and label_off[b + 1] are uniform per workgroup: scalar loads. The image's labels go through
// LDS in chunks of CHUNK: a lane converts one label to (box, class, area) and every lane then reads the same label at
// the same time (a broadcast, no bank conflicts). A lane keeps its running (bi, best) in registers and updates them
// with >=, labels ascending, so the tie rule holds across chunks. A pair whose intersection is empty or whose classes
// differ has IoU 0 (or NaN, which the reference never accepts either) and cannot be a maximum > 0: it skips the
// division. Then (bi, best) of all rows go to LDS and row d scans the rows before it for m[d]. Every byte of tp is
// written once, by the lane of its row; no atomics, nothing depends on timing. No LDS array is indexed by label and
// nothing is kept per label: the number of labels per image is unbounded.
#include "common.h"

namespace ys {

namespace ematch {
constexpr int CHUNK = 256;   // labels staged per pass (_hip.EVAL_MATCH_LABEL_CHUNK says the same)
constexpr int MAX_D = 1024;  // detection rows per image (one lane each)
constexpr int MAX_T = 16;    // thresholds, by value in the kernel arguments
struct Thr {
  float v[MAX_T];
};
}  // namespace ematch

__global__ __launch_bounds__(1024) void eval_match_kernel(const float* __restrict__ det,
                                                          const int* __restrict__ counts, int D,
                                                          const float* __restrict__ labels,
                                                          const int* __restrict__ label_off, ematch::Thr thr, int T,
                                                          uint8_t* __restrict__ tp) {
  using namespace ematch;
  __shared__ float4 s_box[CHUNK];  // x1, y1, x2, y2 of the staged labels
  __shared__ float2 s_ca[CHUNK];   // class, area
  __shared__ float2 s_row[MAX_D];  // bi, best (bit pattern) of every row
  const int b = blockIdx.x, d = threadIdx.x;
  const int count = min(max(counts[b], 0), D);
  const int lo = label_off[b], hi = label_off[b + 1];
  const int nl = (labels != nullptr && hi > lo) ? hi - lo : 0;
  const bool live = d < count;
  float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, dc = 0.f, da = 0.f;
  if (live) {
    const float* r = det + ((size_t)b * D + d) * 6;
    x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3], dc = r[5];
    da = (x2 - x1) * (y2 - y1);
  }
  float bi = 0.f;
  int best = -1;
  for (int c0 = 0; c0 < nl; c0 += CHUNK) {
    const int n = min(CHUNK, nl - c0);
    __syncthreads();  // the previous chunk has been read by every wave
    for (int j = d; j < n; j += blockDim.x) {
      const float* l = labels + ((size_t)lo + c0 + j) * 5;
      const float lx1 = l[1], ly1 = l[2], lx2 = l[3], ly2 = l[4];
      s_box[j] = make_float4(lx1, ly1, lx2, ly2);
      s_ca[j] = make_float2(l[0], (lx2 - lx1) * (ly2 - ly1));
    }
    __syncthreads();
    if (live) {
      for (int j = 0; j < n; ++j) {
        const float4 lb = s_box[j];
        const float2 ca = s_ca[j];
        const float w = fmaxf(fminf(lb.z, x2) - fmaxf(lb.x, x1), 0.f);
        const float h = fmaxf(fminf(lb.w, y2) - fmaxf(lb.y, y1), 0.f);
        const float inter = w * h;
        if (ca.x == dc && inter > 0.f) {
          const float iou = inter / (((ca.y + da) - inter) + 1e-7f);
          if (iou >= bi) {  // >=: of equal maxima the highest label index stays
            bi = iou;
            best = c0 + j;
          }
        }
      }
    }
  }
  if (!(bi > 0.f)) best = -1;
  s_row[d] = make_float2(bi, __int_as_float(best));
  __syncthreads();
  float m = 0.f;
  if (best >= 0) {
    for (int e = 0; e < d; ++e) {  // active lanes read the same row: a broadcast
      const float2 r = s_row[e];
      if (__float_as_int(r.y) == best) m = fmaxf(m, r.x);
    }
  }
  if (d < D) {
    uint8_t* o = tp + ((size_t)b * D + d) * T;
#pragma unroll
    for (int t = 0; t < MAX_T; ++t)
      if (t < T) o[t] = (bi >= thr.v[t] && thr.v[t] > m) ? 1 : 0;
  }
}

}  // namespace ys

using namespace ys;

YS_EXPORT int yolosod_match_predictions(const float* det, const int* counts, int B, int D, const float* labels,
                                        const int* label_off, const float* iouv, int T, uint8_t* tp, void* stream) {
  using namespace ematch;
  YS_CHECK_ARG(det && counts && label_off && iouv && tp, "match_predictions: null pointer");
  YS_CHECK_ARG(B >= 1, "match_predictions: B=%d", B);
  YS_CHECK_ARG(D >= 1 && D <= MAX_D, "match_predictions: D=%d unsupported (1..%d)", D, MAX_D);
  YS_CHECK_ARG(T >= 1 && T <= MAX_T, "match_predictions: T=%d unsupported (1..%d)", T, MAX_T);
  Thr thr;
  for (int t = 0; t < MAX_T; ++t) thr.v[t] = 0.f;
  for (int t = 0; t < T; ++t) {
    const float v = iouv[t];
    YS_CHECK_ARG(v > 0.f && v <= 3.402823466e+38f, "match_predictions: threshold %d is %g (finite and > 0 expected)",
                 t, (double)v);
    thr.v[t] = v;
  }
  YS_CHECK_ARG(((uintptr_t)det & 3) == 0 && ((uintptr_t)counts & 3) == 0 && ((uintptr_t)labels & 3) == 0 &&
                   ((uintptr_t)label_off & 3) == 0,
               "match_predictions: misaligned pointer");
  const unsigned block = (unsigned)((D + 63) / 64 * 64);
  hipLaunchKernelGGL(eval_match_kernel, dim3((unsigned)B), dim3(block), 0, (hipStream_t)stream, det, counts, D, labels,
                     label_off, thr, T, tp);
  YS_CHECK_LAUNCH("match_predictions");
  return 0;
}
