// Validation's second result: the confusion matrix of a batch of padded NMS rows against its labels
// (ultralytics/utils/metrics.py:326-382 ConfusionMatrix.process_batch, detect task, over metrics.py:52-71 box_iou), one
// launch for the batch and no host sync. The sibling of eval_match.hip: same geometry, same box_iou, another rule.
//
// The reference takes the pairs with IoU > iou_thr, sorts them by IoU, keeps each detection's best label (np.unique
// over detections) and then each label's best claimant (a second sort and np.unique over labels). Its result for one
// image with labels l = 0..L-1 and rows d = 0..n-1 in NMS order is exactly (tests/confusion_ref.py):
//   kept(d)    conf[d] > conf_thr                                 (fp32; NaN is not kept)
//   dc[d], gc[l]  the fp32 class truncated to int
//   iou[l][d]  box_iou as in eval_match.hip (fp32, one rounding per operation, no FMA contraction: this file is built
//              with -ffp-contract=off; IEEE division; + 1e-7f), class-agnostic
//   v[d], bl[d]   v[d] = max_l iou[l][d] over the pairs with iou[l][d] > iou_thr (strict); bl[d] the label that attains
//              it, the highest index on a tie; none if no pair passes
//   win(d)     bl[d] exists and no kept e != d has bl[e] == bl[d] with v[e] > v[d], or v[e] == v[d] and e > d
//   M[dc[d]][gc[bl[d]]] += 1  for every kept d with win(d)
//   M[dc[d]][nc]        += 1  for every kept d without win(d)
//   M[nc][gc[l]]        += 1  for every label l that no winner claims
// M is [nc+1][nc+1], rows the predicted class, columns the true class, index nc the background.
//
// One workgroup per image, one lane per detection row (D <= 1024 rows, the block is D rounded up to whole waves).
// counts[b], label_off[b] and label_off[b + 1] are uniform per workgroup. The image's labels go through LDS in chunks of
// CHUNK: a lane converts one label to (box, class, area) and every lane then reads the same label at the same time (a
// broadcast). A lane keeps its running (v, bl, gc[bl]) in registers and updates them with >=, labels ascending, so the
// tie rule holds across chunks. A pair whose intersection is empty (or NaN) cannot pass a threshold >= 0 and skips the
// division. Then (v, bl) of all rows go to LDS and row d scans the other rows for a better claimant of its label.
// Nothing is indexed or kept per label: the number of labels per image is unbounded.
//
// Counting happens in an LDS matrix of (nc+1)^2 int32 per workgroup: the staging lane of a label adds it to M[nc][gc]
// (missed until claimed), a winner moves that count to M[dc][gc], a kept row that does not win adds to M[dc][nc]. Only
// integer LDS atomics: the sums do not depend on order. The finished matrix goes to cm[b] with plain stores, every cell
// written exactly once; no global atomics, no pre-zeroed output.
//
// A row or label whose class is NaN or truncates outside [0, nc) is counted nowhere and writes nothing (the reference
// would raise an IndexError there, or wrap a negative index); it still takes part in the matching: such a row can take
// a label from another row, and a winner of such a label is counted nowhere while the label is not counted as missed.
#include "common.h"

namespace ys {

namespace econf {
constexpr int CHUNK = 256;   // labels staged per pass (_hip.EVAL_CONFUSION_LABEL_CHUNK says the same)
constexpr int MAX_D = 1024;  // detection rows per image (one lane each)
constexpr int MAX_NC = 100;  // classes (_hip.EVAL_CONFUSION_MAX_NC): the LDS matrix is (MAX_NC + 1)^2 int32 = 40804 B
constexpr int MAX_CELLS = (MAX_NC + 1) * (MAX_NC + 1);

// the class as an index: a value in (-1, nc) truncates (toward zero) into [0, nc); everything else, NaN included, is -1
__device__ __forceinline__ int class_index(float c, int nc) { return (c > -1.f && c < (float)nc) ? (int)c : -1; }
}  // namespace econf

__global__ __launch_bounds__(1024) void eval_confusion_kernel(const float* __restrict__ det,
                                                              const int* __restrict__ counts, int D,
                                                              const float* __restrict__ labels,
                                                              const int* __restrict__ label_off, int nc,
                                                              float conf_thr, float iou_thr, int* __restrict__ cm) {
  using namespace econf;
  __shared__ float4 s_box[CHUNK];  // x1, y1, x2, y2 of the staged labels
  __shared__ float2 s_ga[CHUNK];   // class index (bit pattern), area
  __shared__ float2 s_row[MAX_D];  // v, bl (bit pattern) of every row
  __shared__ int s_m[MAX_CELLS];   // the image's matrix, [nc+1][nc+1]
  const int b = blockIdx.x, d = threadIdx.x;
  const int nc1 = nc + 1, cells = nc1 * nc1;
  const int count = min(max(counts[b], 0), D);
  const int lo = label_off[b], hi = label_off[b + 1];
  const int nl = (labels != nullptr && hi > lo) ? hi - lo : 0;
  for (int i = d; i < cells; i += blockDim.x) s_m[i] = 0;
  float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, da = 0.f;
  bool kept = false;
  int dci = -1;
  if (d < count) {
    const float* r = det + ((size_t)b * D + d) * 6;
    x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
    kept = r[4] > conf_thr;
    dci = class_index(r[5], nc);
    da = (x2 - x1) * (y2 - y1);
  }
  float v = 0.f;
  int bl = -1, g = -1;
  for (int c0 = 0; c0 < nl; c0 += CHUNK) {
    const int n = min(CHUNK, nl - c0);
    __syncthreads();  // the matrix is zeroed; the previous chunk has been read by every wave
    for (int j = d; j < n; j += blockDim.x) {
      const float* l = labels + ((size_t)lo + c0 + j) * 5;
      const float lx1 = l[1], ly1 = l[2], lx2 = l[3], ly2 = l[4];
      const int gci = class_index(l[0], nc);
      s_box[j] = make_float4(lx1, ly1, lx2, ly2);
      s_ga[j] = make_float2(__int_as_float(gci), (lx2 - lx1) * (ly2 - ly1));
      if (gci >= 0) atomicAdd(&s_m[nc * nc1 + gci], 1);  // missed, until a winner claims it
    }
    __syncthreads();
    if (kept) {
      for (int j = 0; j < n; ++j) {
        const float4 lb = s_box[j];
        const float2 ga = s_ga[j];
        const float w = fmaxf(fminf(lb.z, x2) - fmaxf(lb.x, x1), 0.f);
        const float h = fmaxf(fminf(lb.w, y2) - fmaxf(lb.y, y1), 0.f);
        const float inter = w * h;
        if (inter > 0.f) {
          const float iou = inter / (((ga.y + da) - inter) + 1e-7f);
          if (iou > iou_thr && iou >= v) {  // >=: of equal maxima the highest label index stays
            v = iou;
            bl = c0 + j;
            g = __float_as_int(ga.x);
          }
        }
      }
    }
  }
  s_row[d] = make_float2(v, __int_as_float(bl));  // rows that are not kept: bl = -1, they claim nothing
  __syncthreads();
  if (kept) {
    bool win = bl >= 0;
    if (win) {
      for (int e = 0; e < count; ++e) {  // active lanes read the same row: a broadcast
        const float2 r = s_row[e];
        if (__float_as_int(r.y) == bl && (r.x > v || (r.x == v && e > d))) win = false;
      }
    }
    if (win) {
      if (g >= 0) {
        atomicSub(&s_m[nc * nc1 + g], 1);
        if (dci >= 0) atomicAdd(&s_m[dci * nc1 + g], 1);
      }
    } else if (dci >= 0) {
      atomicAdd(&s_m[dci * nc1 + nc], 1);
    }
  }
  __syncthreads();
  int* o = cm + (size_t)b * cells;
  for (int i = d; i < cells; i += blockDim.x) o[i] = s_m[i];
}

}  // namespace ys

using namespace ys;

YS_EXPORT int yolosod_confusion_matrix(const float* det, const int* counts, int B, int D, const float* labels,
                                       const int* label_off, int nc, float conf_thr, float iou_thr, int32_t* cm,
                                       void* stream) {
  using namespace econf;
  YS_CHECK_ARG(det && counts && label_off && cm, "confusion_matrix: null pointer");
  YS_CHECK_ARG(B >= 1, "confusion_matrix: B=%d", B);
  YS_CHECK_ARG(D >= 1 && D <= MAX_D, "confusion_matrix: D=%d unsupported (1..%d)", D, MAX_D);
  YS_CHECK_ARG(nc >= 1 && nc <= MAX_NC, "confusion_matrix: nc=%d unsupported (1..%d)", nc, MAX_NC);
  YS_CHECK_ARG(conf_thr >= 0.f && conf_thr <= 3.402823466e+38f,
               "confusion_matrix: conf_thr is %g (finite and >= 0 expected)", (double)conf_thr);
  YS_CHECK_ARG(iou_thr >= 0.f && iou_thr <= 3.402823466e+38f,
               "confusion_matrix: iou_thr is %g (finite and >= 0 expected)", (double)iou_thr);
  YS_CHECK_ARG(((uintptr_t)det & 3) == 0 && ((uintptr_t)counts & 3) == 0 && ((uintptr_t)labels & 3) == 0 &&
                   ((uintptr_t)label_off & 3) == 0 && ((uintptr_t)cm & 3) == 0,
               "confusion_matrix: misaligned pointer");
  const unsigned block = (unsigned)((D + 63) / 64 * 64);
  hipLaunchKernelGGL(eval_confusion_kernel, dim3((unsigned)B), dim3(block), 0, (hipStream_t)stream, det, counts, D,
                     labels, label_off, nc, conf_thr, iou_thr, cm);
  YS_CHECK_LAUNCH("confusion_matrix");
  return 0;
}
