/*
 * yolosod_hip.h - C ABI of the MI355X (gfx950) hot path of YOLO-SOD inference.
 *
 * Library: yolo-sod_amd/lib/libyolosod_hip.so  (built by `python -m yolosod_amd.build` / __graft_entry__.build()).
 *
 * Conventions (every entry point):
 *   - all tensor arguments are DEVICE pointers to contiguous fp32 (or int32) buffers in the reference's layout
 *     (NCHW feature maps, PyTorch Linear/Conv weight layouts), allocated and owned by the caller;
 *   - `workspace` is a caller-owned device buffer of at least yolosod_<op>_workspace(...) bytes;
 *   - `stream` is a hipStream_t; launches are stream-ordered, nothing synchronises the host;
 *   - return 0 on success, nonzero on error (message in yolosod_last_error(), thread-local).
 *   - outputs never alias inputs, except yolosod_nms with in_place=1 which rewrites pred[:, 0:4] to xyxy,
 *     mirroring non_max_suppression(in_place=True).
 *
 * Each entry point replaces one reference interface (quitedob/yolo-sod, file:line):
 */
#ifndef YOLOSOD_HIP_H
#define YOLOSOD_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int yolosod_abi_version(void);
const char* yolosod_last_error(void);
/* Per-device state (the split-range flag word), allocated and zeroed eagerly; idempotent. Call once per device before
 * the first launch on it (and before any stream capture): a launch on a device never initialised allocates the state
 * itself, synchronously. Returns 0, or < 0 on error. The current device is restored. */
int yolosod_init(int device);

/* SE / SE_Block.forward            ultralytics/nn/modules/smallobj_modules.py:84-92
 * y = x * sigmoid(fc2(relu(fc1(mean_hw(x)))));  fc1: [hidden,C]+[hidden], fc2: [C,hidden]+[C]. */
size_t yolosod_se_workspace(int B, int C, int H, int W);
int yolosod_se_forward(const float* x, float* y, int B, int C, int H, int W, const float* fc1_w, const float* fc1_b,
                       const float* fc2_w, const float* fc2_b, int hidden, void* workspace, size_t workspace_bytes,
                       void* stream);

/* CBAM_Block.forward               ultralytics/nn/modules/cbam_block.py:52-55 (ChannelAttention :19-23,
 * SpatialAttention :32-37).  fc0: [hidden,C] (channel_attention.fc.0), fc2: [C,hidden] (fc.2), sa_w: [1,2,7,7]. */
size_t yolosod_cbam_workspace(int B, int C, int H, int W);
int yolosod_cbam_forward(const float* x, float* y, int B, int C, int H, int W, const float* fc0_w,
                         const float* fc2_w, int hidden, const float* sa_w, void* workspace, size_t workspace_bytes,
                         void* stream);

/* CA_Block.forward                 ultralytics/nn/modules/ca_block.py:38-59 (bn1 in eval mode, not fused). */
size_t yolosod_ca_workspace(int B, int C, int H, int W);
int yolosod_ca_forward(const float* x, float* y, int B, int C, int H, int W, const float* conv1_w,
                       const float* conv1_b, int mip, const float* bn_w, const float* bn_b, const float* bn_mean,
                       const float* bn_var, float bn_eps, const float* convh_w, const float* convh_b,
                       const float* convw_w, const float* convw_b, void* workspace, size_t workspace_bytes,
                       void* stream);

/* A2_Attn.forward (Conv layers in fused form, nn/tasks.py:227-255)   ultralytics/nn/modules/a2_attn.py:35-69
 * proj / oproj: [C,C] fused conv weight + bias (SiLU), MHA: in_proj [3C,C]+[3C], out_proj [C,C]+[C]. */
size_t yolosod_a2_workspace(int B, int C, int H, int W, int num_areas);
int yolosod_a2_forward(const float* x, float* y, int B, int C, int H, int W, int num_areas, int num_heads,
                       const float* proj_w, const float* proj_b, const float* ln_w, const float* ln_b, float ln_eps,
                       const float* in_proj_w, const float* in_proj_b, const float* mha_out_w,
                       const float* mha_out_b, const float* oproj_w, const float* oproj_b, void* workspace,
                       size_t workspace_bytes, void* stream);
/* The fused LN -> QKV -> attention kernel of the fp16-split path (csrc/a2_fused.hip; head dim 64, areas * W <= 160)
 * and the proj + SiLU + pooling kernel (area groups whose rows fit 400 pixels; any sequence length) take the weights
 * prepared once: yolosod_a2_prep_bytes (0 = the shape takes neither fused kernel), yolosod_a2_prepare (in_proj with the LayerNorm affine folded and the
 * BN-folded proj conv, split into fp16 planes; re-run when one of them changes), yolosod_a2_forward_prepared (the forward of yolosod_a2_forward with the pre-multiplied output
 * weights, on that block; the workspace is yolosod_a2_workspace). yolosod_a2_forward prepares per call instead. */
size_t yolosod_a2_prep_bytes(int C, int num_heads, int num_areas, int W);
int yolosod_a2_prepare(int C, const float* proj_w, const float* ln_w, const float* ln_b, const float* in_proj_w,
                       const float* in_proj_b, void* prep, size_t prep_bytes, void* stream);
int yolosod_a2_forward_prepared(const float* x, float* y, int B, int C, int H, int W, int num_areas, int num_heads,
                                const float* proj_w, const float* proj_b, const float* ln_w, const float* ln_b,
                                float ln_eps, const float* in_proj_w, const float* in_proj_b, const float* oproj_w,
                                const float* oproj_b, const void* prep, size_t prep_bytes, void* workspace,
                                size_t workspace_bytes, void* stream);

/* SwinBlock.forward                ultralytics/nn/modules/blocks_transformer.py:150-171 (WindowAttention
 * :100-131, window_partition :8-47, window_reverse :49-79).  dw: [C,1,3,3]; in_proj [3C,C]; mlp1 [hid,C];
 * mlp2 [C,hid]; pw [C,C,1,1]; bn in eval mode (not fused by fuse()). */
size_t yolosod_swin_workspace(int B, int C, int H, int W, int window, int mlp_hidden);
/* heads-aware query: small when the fused per-window kernel handles the shape (C in {32,64,128}, <=49 tokens) */
size_t yolosod_swin_workspace_v2(int B, int C, int H, int W, int num_heads, int window, int mlp_hidden);
int yolosod_swin_forward(const float* x, float* y, int B, int C, int H, int W, int num_heads, int window,
                         const float* dw_w, const float* ln1_w, const float* ln1_b, float ln1_eps,
                         const float* in_proj_w, const float* in_proj_b, const float* out_proj_w,
                         const float* out_proj_b, const float* ln2_w, const float* ln2_b, float ln2_eps,
                         const float* mlp1_w, const float* mlp1_b, int mlp_hidden, const float* mlp2_w,
                         const float* mlp2_b, const float* pw_w, const float* bn_w, const float* bn_b,
                         const float* bn_mean, const float* bn_var, float bn_eps, void* workspace,
                         size_t workspace_bytes, void* stream);
/* The same forward with the parameter preparation (weight split into fp16 planes with the LayerNorm affines folded,
 * BN fold) done once by the caller and kept across calls, for the shapes of the fp16-split kernels (7x7 windows,
 * C = 64 / 2 heads and C = 256 / 4 heads, mlp_hidden = 2C): yolosod_swin_prep_bytes returns the block's size (0 when
 * (C, heads, hidden) has no such kernel), yolosod_swin_prepare fills a caller-owned block from the parameters of
 * yolosod_swin_forward (re-run it whenever a parameter changes), yolosod_swin_forward_prepared runs the block with a
 * caller-owned scratch of yolosod_swin_prepared_workspace bytes (C = 64: T after the attention residual, token-major,
 * between the attention kernel and the token-tiled MLP kernel). The block also keeps the weights' split-range result,
 * which every forward on it reports again (yolosod_split_range_flag). One image's C*H*W must stay below 2^30. */
size_t yolosod_swin_prep_bytes(int C, int num_heads, int mlp_hidden);
size_t yolosod_swin_prepared_workspace(int B, int C, int H, int W, int num_heads, int window, int mlp_hidden);
int yolosod_swin_prepare(int C, int num_heads, int mlp_hidden, const float* ln1_w, const float* ln1_b,
                         const float* in_proj_w, const float* in_proj_b, const float* out_proj_w, const float* ln2_w,
                         const float* ln2_b, const float* mlp1_w, const float* mlp1_b, const float* mlp2_w,
                         const float* pw_w, const float* bn_w, const float* bn_b, const float* bn_mean,
                         const float* bn_var, float bn_eps, void* prep, size_t prep_bytes, void* stream);
int yolosod_swin_forward_prepared(const float* x, float* y, int B, int C, int H, int W, int num_heads, int window,
                                  const float* dw_w, float ln1_eps, const float* out_proj_b, float ln2_eps,
                                  int mlp_hidden, const float* mlp2_b, const void* prep, size_t prep_bytes,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* Producer-side statistics for the channel gates (SE smallobj_modules.py:87, CBAM cbam_block.py:14-17): a conv
 * epilogue that also writes its output's per-plane partial sums (+ maxes when pmax != NULL) in the segmentation
 * yolosod_plane_parts returns (parts per plane, floats per part), and SE / CBAM entry points that take them instead
 * of re-reading x (bitwise the same gate inputs up to summation order). */
int yolosod_plane_parts(long HW, long* seg);
int yolosod_bias_act_stats(const float* y, long y_bstride, float* out, long out_bstride, const float* bias,
                           const float* res, long res_bstride, int B, int C, long HW, int act, int parts, long seg,
                           float* psum, float* pmax, void* stream);
int yolosod_se_forward_pre(const float* x, float* y, int B, int C, int H, int W, const float* fc1_w,
                           const float* fc1_b, const float* fc2_w, const float* fc2_b, int hidden, const float* psum,
                           void* workspace, size_t workspace_bytes, void* stream);
int yolosod_cbam_forward_pre(const float* x, float* y, int B, int C, int H, int W, const float* fc0_w,
                             const float* fc2_w, int hidden, const float* sa_w, const float* psum, const float* pmax,
                             void* workspace, size_t workspace_bytes, void* stream);
/* CA_Block (ca_block.py:43-44): the producing conv's epilogue also writes the pooled row means (over W) and column
 * means (over H) of its output, yin[B][C][H+W]; the CA entry point then runs the gate and the apply pass only.
 * W % 4 == 0, W <= 1024. */
int yolosod_bias_act_capool(const float* y, long y_bstride, float* out, long out_bstride, const float* bias,
                            const float* res, long res_bstride, int B, int C, int H, int W, int act, float* yin,
                            void* stream);
/* Nearest 2x upsample (nn.Upsample(None, 2, 'nearest') rows of the neck YAML) of x [B, C, h, w] into a channel
 * slice of the following Concat's buffer (out batch stride in elements): the neck glue's copy, not a hot-path op.
 * elem_bytes 4 (fp32) / 2 (bf16); w % 4 == 0 and 16-byte aligned pointers / strides. */
int yolosod_upsample2x(const void* x, void* out, long out_bstride, int B, int C, int h, int w, int elem_bytes,
                       void* stream);
/* The stem (layer 0: Conv 3 -> Cout, 3x3, stride 2, pad 1, SiLU) as one streaming pass: out [B, Cout, H/2, W/2] =
 * SiLU(conv(x [B, 3, H, W], w [Cout, 3, 3, 3]) + bias), contiguous fp32, exact fp32 FMAs in (ci, ky, kx) order, plus
 * the output's per-plane partial sums psum [B * Cout * parts] in the yolosod_plane_parts(H/2 * W/2) segmentation for
 * the SE that follows (as yolosod_bias_act_stats emits them). H even, (W/2) % 4 == 0, Cout even and <= 64, x / out
 * 16-byte aligned; workspace: yolosod_stem_workspace bytes of tile partials. Deterministic (no atomics). */
size_t yolosod_stem_workspace(int B, int Cout, int H, int W);
int yolosod_stem_conv(const float* x, const float* w, const float* bias, float* out, int B, int Cout, int H, int W,
                      int parts, long seg, float* psum, void* workspace, size_t workspace_bytes, void* stream);
int yolosod_ca_forward_pre(const float* x, float* y, int B, int C, int H, int W, const float* conv1_w,
                           const float* conv1_b, int mip, const float* bn_w, const float* bn_b, const float* bn_mean,
                           const float* bn_var, float bn_eps, const float* convh_w, const float* convh_b,
                           const float* convw_w, const float* convw_b, const float* yin, void* workspace,
                           size_t workspace_bytes, void* stream);

/* MambaBlock (GLU fallback)        ultralytics/nn/modules/blocks_mamba.py:84-113 (Conv1x1BN, GLUBlock), :198-236
 * (forward without mamba_ssm); arg rule nn/tasks.py:1122-1127 (MambaBlock(c, c_hidden, seq_reduction)).
 * y = x + SiLU(BN_o(W_o . up_nearest(GLU(avg_pool_r(SiLU(BN_i(W_i . x)))))))  with
 * GLU(p) = W_pw2 . SiLU(BN(dw3x3(sigmoid(g) * a))), [a; g] = W_pw1 . p. All BatchNorms in eval form (not folded by
 * the reference's fuse()). x, y: [B, C, H, W]; c_hidden = ch; reduction r >= 1 (pool kernel = stride = r, floor;
 * nearest upsample back to H x W). C and ch multiples of 32. */
size_t yolosod_mamba_glu_workspace(int B, int C, int H, int W, int ch, int reduction);
int yolosod_mamba_glu_forward(const float* x, float* y, int B, int C, int H, int W, int ch, int reduction,
                              const float* in_w, const float* in_bn_w, const float* in_bn_b, const float* in_bn_mean,
                              const float* in_bn_var, float in_bn_eps, const float* pw1_w, const float* dw_w,
                              const float* bn_w, const float* bn_b, const float* bn_mean, const float* bn_var,
                              float bn_eps, const float* pw2_w, const float* out_w, const float* out_bn_w,
                              const float* out_bn_b, const float* out_bn_mean, const float* out_bn_var,
                              float out_bn_eps, void* workspace, size_t workspace_bytes, void* stream);

/* Detect._inference (decode)       ultralytics/nn/modules/head.py:100-131, DFL block.py:79-82,
 * make_anchors / dist2bbox utils/tal.py:333-357.
 * maps: host array of nl device pointers, map i = [B, 4*reg_max+nc, heights[i], widths[i]];
 * y: [B, 4+nc, A] (xywh * stride, sigmoid scores), A = sum_i heights[i]*widths[i]. */
int yolosod_detect_decode(int nl, const float* const* maps, const int* heights, const int* widths,
                          const float* strides, int B, int nc, int reg_max, float* y, void* stream);

/* Detect head tail fused with the decode (head.py:45-48,70 + the decode above): the last 1x1 convs
 * of the box tower (box_w [64][c2], box_b [64]) and class tower (cls_w [nc][c3], cls_b [nc]) applied to the tower
 * features box_feat[i] [B][c2][H_i][W_i], cls_feat[i] [B][c3][H_i][W_i] (fp32 NCHW, contiguous), then DFL /
 * dist2bbox / sigmoid -> y [B][4+nc][A]; the [B][64+nc][H][W] raw maps are never materialised.
 * Supports reg_max 16, c2 64, c3 64 or 128, nc <= 16. */
int yolosod_detect_head(int nl, const float* const* box_feat, const float* const* cls_feat, int c2, int c3,
                        const float* const* box_w, const float* const* box_b, const float* const* cls_w,
                        const float* const* cls_b, const int* heights, const int* widths, const float* strides, int B,
                        int nc, int reg_max, float* y, void* stream);

/* non_max_suppression + torchvision.ops.nms   ultralytics/utils/ops.py:167-316 (nms call :296).
 * pred: [B, 4+nc, A] xywh (rewritten to xyxy in place when in_place); classes: device int32[n_classes] or NULL;
 * out: [B, max_det, 6] rows (x1,y1,x2,y2,conf,cls) in kept order, zero padded; counts: [B];
 * out_index: [B, max_det] anchor index of each kept row (-1 padded). max_det 1..2^20 (the reference has no cap,
 * ops.py:297); the workspace depends on max_det above 1024 (_v2), the original query covers max_det <= 1024. */
size_t yolosod_nms_workspace(int B, int nc, int A, int multi_label);
size_t yolosod_nms_workspace_v2(int B, int nc, int A, int multi_label, int max_det);
int yolosod_nms(float* pred, int B, int nc, int A, float conf_thres, double iou_thres, const int* classes,
                int n_classes, int agnostic, int multi_label, int max_det, int max_nms, float max_wh, int in_place,
                float* out, int* counts, int* out_index, void* workspace, size_t workspace_bytes, void* stream);
/* Merge-NMS (the project's own definition, after the commented-out block ultralytics/utils/ops.py:299-309):
 * yolosod_nms, then one more launch that replaces the box of every kept row k < counts[b] by the score-weighted mean
 * of its cluster. Same arguments, workspace query and launches as yolosod_nms, plus n_merged: [B, max_det] int32.
 *   - candidates: all of the image's candidates as NMS defines them (score > conf_thres, the class filter, best
 *     class or with multi_label every class above conf_thres) - all n of them, not only the max_nms highest, and
 *     without the reference comment's n < 3000 gate;
 *   - membership: candidate j belongs to row k when NMS's own test says k would suppress it: torchvision's formula
 *     in fp32 on the class-offset boxes (box + cls * max_wh, no offset with agnostic),
 *     inter / ((area_k + area_j) - inter) > iou_thres (the comparison against the double threshold);
 *   - row k's own candidate (its anchor and class) is always a member, also when its IoU with itself is NaN (a
 *     zero-area box): the weight sum is never 0;
 *   - merged coordinate c of x1, y1, x2, y2 (plain xyxy, no offset): sum_j (double)score_j * (double)c_j /
 *     sum_j (double)score_j, accumulated and divided in fp64, rounded once to fp32; fixed summation order, no
 *     atomics: two calls on the same input give the same bits;
 *   - conf, cls, out_index, counts and the row order stay as NMS left them; rows >= counts[b] stay zero;
 *   - n_merged[b][k]: the cluster's size, >= 1 for kept rows, 0 for padding (the reference's `redundant` filter
 *     is n_merged > 1; it is not applied here).
 * A cluster of one returns the kept box bit for bit ((s * c) / s is exact), so iou_thres = 1.0 is plain NMS.
 * max_det 1..1024 (larger values are refused; yolosod_nms keeps its full range). */
int yolosod_nms_merged(float* pred, int B, int nc, int A, float conf_thres, double iou_thres, const int* classes,
                       int n_classes, int agnostic, int multi_label, int max_det, int max_nms, float max_wh,
                       int in_place, float* out, int* counts, int* out_index, int* n_merged, void* workspace,
                       size_t workspace_bytes, void* stream);

/* BasePredictor.preprocess, non-tensor branch + LetterBox   ultralytics/engine/predictor.py:116-134, pre_transform
 * :145-161 (LetterBox: ultralytics/data/augment.py, restated in yolo-sod_amd/data/augment.py), one launch per batch.
 * desc: device int64 [B][8] = source address, h, w, row pitch in bytes, new_h, new_w, top, left of each frame: uint8
 * HWC, 3 bytes per pixel in B, G, R order, pitch >= 3*w (a cropped view is a valid frame), h and w <= 16384; frames
 * of one batch may differ in size. The kernel reads whole aligned dwords that hold a byte of the frame.
 * out: [B][3][out_h][out_w] RGB planes, image b at out + b*out_bstride elements (out_bstride % 4 == 0), fp32 or
 * (out_bf16) bf16 bit patterns, out_w % 4 == 0, 16-byte aligned; every element is written: the frame resized to
 * new_h x new_w at (top, left) (integer bilinear, csrc/ingest.hip; value = float(q) / 255.0f, bf16 rounded once
 * more to nearest even), pad_value / 255 elsewhere. Deterministic. */
int yolosod_letterbox_ingest(const int64_t* desc, int B, void* out, long out_bstride, int out_h, int out_w,
                             int out_bf16, int pad_value, void* stream);
/* The same front door for decoded video (the project's own: the reference reads BGR frames only): NV12 surfaces -> the
 * input tensor, one launch per batch (csrc/ingest_nv12.hip). desc: device int64 [B][12] per frame =
 *   0 Y address of the view's first pixel, 1 UV address of that pixel's chroma pair (row y0 >> 1, pair x0 >> 1 of the
 *   surface), 2 h, 3 w of the view (1..16384, odd extents allowed), 4 Y pitch, 5 UV pitch in bytes, 6 new_h, 7 new_w,
 *   8 top, 9 left, 10 the parities of the view's origin on its surface (y0 & 1) << 1 | (x0 & 1), 11 matrix id:
 *   0 bt601, 1 bt709 (limited range), 2 bt601_full, 3 bt709_full.
 * View pixel (r, c) takes Y[r][c] and the pair U, V at chroma row (r + py) >> 1, pair (c + px) >> 1 from field 1 (no
 * chroma interpolation) and becomes uint8 B, G, R in int32 arithmetic (the table and formula are in
 * csrc/ingest_nv12.hip); those pixels then take yolosod_letterbox_ingest's resize, border, / 255 and bf16 rounding:
 * the result is bit-equal to yolosod_letterbox_ingest on the converted frames. A frame with h < 1 or w < 1 is not
 * read: its image is all border. The kernel reads whole aligned dwords that hold a byte of the view's Y rows or of
 * their chroma pairs. out and the remaining arguments as yolosod_letterbox_ingest. Deterministic. */
int yolosod_letterbox_ingest_nv12(const int64_t* desc, int B, void* out, long out_bstride, int out_h, int out_w,
                                  int out_bf16, int pad_value, void* stream);
/* DetectionPredictor.postprocess -> scale_boxes  ultralytics/models/yolo/detect/predict.py:23-41,
 * ultralytics/utils/ops.py:92-128 (clip_boxes :319-338) on the padded NMS output with per-image geometry, no host
 * sync. det: [B][D][6]; geom: device float [B][5] = gain, pad_x, pad_y, w0, h0. Rows < counts[b]: columns 0..3
 * become (v - pad) / gain (IEEE division) clamped to [0, w0] / [0, h0]; rows >= counts[b] and columns 4, 5 are not
 * touched. D in 1..2^20. */
int yolosod_scale_boxes(float* det, const int* counts, int B, int D, const float* geom, void* stream);
/* Sliced inference (the project's own: the reference has no slicing), the step between the Detect head and NMS, one
 * launch per model call. y: [n][4+nc][A] fp32, the head's output for n tiles letterboxed onto one canvas (xywh in
 * canvas pixels, sigmoid scores). merged: [F][4+nc][S*A] fp32, one prediction tensor per frame in frame pixels, slot s
 * at anchors [s*A, (s+1)*A). desc: device int32 [rows][16], one row per destination slot this call writes:
 *   0 src (row of y; -1: the slot is empty, zeros are written), 1 frame, 2 slot, 3 flags (bit 0 left, 1 right, 2 top,
 *   3 bottom tile edge interior to the frame), then fp32 bit patterns 4 gain, 5 pad_x, 6 pad_y (scale_boxes' own, of
 *   the tile on the canvas), 7 off_x, 8 off_y (the tile's x0, y0), 9 tile_w, 10 tile_h; 11..15 unused.
 * Per anchor, fp32 with IEEE division: b = (xy - pad) / gain, wh / gain; merged box = b + off, wh; scores are copied,
 * or 0 when cut_margin >= 0 and the box comes within cut_margin of an interior tile edge (csrc/tile_merge.hip). Every
 * element of a named slot is written exactly once, nothing else is touched, no atomics: deterministic. A row naming a
 * src >= n, a frame outside [0, F) or a slot outside [0, S) writes nothing. nc in 1..64, S*A*nc < 2^32, rows in
 * 1..65535; 16-byte accesses when A % 4 == 0 and y, merged are 16-byte aligned. */
int yolosod_tile_merge(const float* y, int n, int nc, int A, const int32_t* desc, int rows, float* merged, int F,
                       int S, float cut_margin, void* stream);
/* Test-time augmentation   ultralytics/nn/tasks.py:381-418 (_predict_augment), utils/torch_utils.py:423-432 (scale_img)
 * (csrc/tta.hip). yolosod_tta_views makes every scaled / flipped view of one batch in one launch. x: [B][C][H][W]
 * contiguous, fp32 or (bf16) bf16 bit patterns. desc: device int64 [V][8] = output address, flip (0 none, 2 up-down,
 * 3 left-right), sh, sw (resized size), ph, pw (padded size), 0, 0; view v is [B][C][ph][pw] contiguous in x's type at
 * its address, 16-byte aligned, pw % 4 == 0, sh <= ph <= max_ph, sw <= pw <= max_pw (the launch is sized by max_ph x
 * max_pw; a row that breaks this writes nothing). Every element of every view is written exactly once: the flipped x
 * resized to sh x sw at the top-left, 0.447f elsewhere. Resize per axis n_in -> n_out in fp32, every operation rounded
 * on its own: scale = float(n_in) / float(n_out); src = max(scale * (d + 0.5f) - 0.5f, 0); i0 = min((int)src,
 * n_in - 1); i1 = i0 + (i0 < n_in - 1); l1 = src - i0; l0 = 1 - l1; a flip replaces index i by n_in - 1 - i on its
 * axis; value = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d). bf16 input is widened first, the fp32 value is
 * rounded once to nearest even. Upscaling included. V * B * C <= 65535, extents <= 16384. Deterministic.
 * yolosod_tta_merge is _descale_pred + _clip_augmented + torch.cat for one branch: anchors [src_lo, src_lo + n) of
 * y [B][4+nc][A] (fp32, the head's output for the view) become anchors [dst, dst + n) of cat [B][4+nc][A_tot]: x, y, w,
 * h each / scale (IEEE division), then x = img_w - x (flip 3) or y = img_h - y (flip 2); scores are copied. Everything
 * in the named range is written exactly once, nothing else is touched, no atomics. nc in 1..64, B <= 65535, scale
 * finite and > 0, the ranges inside y and cat. */
int yolosod_tta_views(const void* x, int B, int C, int H, int W, int bf16, const int64_t* desc, int V, int max_ph,
                      int max_pw, void* stream);
int yolosod_tta_merge(const float* y, int B, int nc, int A, int src_lo, int n, float* cat, int A_tot, int dst,
                      float scale, int flip, float img_w, float img_h, void* stream);
/* Sliced inference with test-time augmentation (the project's own; csrc/tile_merge_tta.hip): one branch of one model
 * call straight into the per-frame prediction tensor, one launch, no concatenated tensor in between. y: [n][4+nc][A]
 * fp32, the head's output for view (scale, flip) of n tiles, in that view's canvas pixels; its anchors [src_lo,
 * src_lo + n_k) go to anchors [slot*A_tot + dst, + n_k) of merged [F][4+nc][S*A_tot] (fp32, frame pixels). desc: device
 * int32 [rows][16], yolosod_tile_merge's descriptor unchanged; (img_w, img_h) the tiles' canvas. Per anchor, fp32, IEEE
 * division, every operation rounded on its own: x, y, w, h each / scale, then x = img_w - x (flip 3) or y = img_h - y
 * (flip 2) (yolosod_tta_merge's arithmetic); on that, (xy - pad) / gain, wh / gain, the cut test against cut_margin on
 * interior edges, + off, scores zeroed where cut (yolosod_tile_merge's). Bit-identical to yolosod_tta_merge into
 * cat [n][4+nc][A_tot] followed by yolosod_tile_merge of cat with A = A_tot. A src = -1 row writes zeros to the
 * branch's range of its slot; over the launches of all branches of one model call every element of every named slot is
 * written exactly once, nothing else is touched, no atomics: deterministic. A row naming a src >= n, a frame outside
 * [0, F) or a slot outside [0, S) writes nothing. nc in 1..64, S*A_tot*nc < 2^32, rows in 1..65535, scale finite and
 * > 0, flip 0 / 2 / 3, the ranges inside y and a slot; 4-byte accesses (A_tot is odd at the workload's shapes). */
int yolosod_tile_merge_tta(const float* y, int n, int nc, int A, int src_lo, int n_k, const int32_t* desc, int rows,
                           float* merged, int F, int S, int A_tot, int dst, float scale, int flip, float img_w,
                           float img_h, float cut_margin, void* stream);
/* BaseValidator.match_predictions over box_iou  ultralytics/engine/validator.py:222-262 (greedy path),
 * ultralytics/utils/metrics.py:52-71, for a whole batch of padded NMS rows in one launch, no host sync
 * (csrc/eval_match.hip). det: [B][D][6] padded NMS rows (x1, y1, x2, y2, conf, cls), counts: device [B]. labels:
 * device [L][5] = cls, x1, y1, x2, y2, the images' labels back to back (may be null when there are none); label_off:
 * device [B+1], label_off[0] = 0, image b owns labels [label_off[b], label_off[b+1]) - the caller vouches that they lie
 * inside labels. iouv: HOST array of T thresholds (they travel by value in the kernel arguments). tp: [B][D][T] bytes.
 * Per image, in fp32 without FMA contraction and with IEEE division: iou = inter / (((a_l + a_d) - inter) + 1e-7f), 0
 * where the classes differ; bi[d] = the best IoU of row d over the labels and best[d] the label that attains it (the
 * highest index on a tie, none if bi[d] == 0); m[d] = the largest bi of an earlier row with the same best label, or 0;
 * tp[d][t] = bi[d] >= iouv[t] && iouv[t] > m[d]. Every byte of tp is written exactly once; rows >= counts[b] and images
 * without labels are 0; no atomics: deterministic. Refused: a null det / counts / label_off / iouv / tp, B < 1, D
 * outside 1..1024, T outside 1..16, a threshold that is <= 0 or not finite. */
int yolosod_match_predictions(const float* det, const int* counts, int B, int D, const float* labels,
                              const int* label_off, const float* iouv, int T, uint8_t* tp, void* stream);
/* ConfusionMatrix.process_batch (detect task) over box_iou  ultralytics/utils/metrics.py:326-382, :52-71, for a whole
 * batch of padded NMS rows in one launch, no host sync (csrc/eval_confusion.hip). det, counts, labels, label_off as
 * for yolosod_match_predictions. cm: [B][nc+1][nc+1] int32, rows the predicted class, columns the true class, index nc
 * the background. Per image, in fp32 without FMA contraction and with IEEE division: a row is kept if conf > conf_thr;
 * iou = inter / (((a_l + a_d) - inter) + 1e-7f) whatever the classes; a kept row's label is the one of its largest
 * iou > iou_thr (the highest index on a tie); a label goes to the kept row that claims it with the largest iou (the
 * highest row on a tie). cm[dc][gc] counts the rows that got their label, cm[dc][nc] the other kept rows, cm[nc][gc]
 * the labels nobody got; dc / gc the fp32 class truncated to int. A row or label whose class is NaN or truncates
 * outside [0, nc) is counted nowhere (it still takes part in the matching). Every cell of cm is written exactly once
 * with plain stores, whatever cm held; integer LDS atomics only: deterministic. Refused: a null det / counts /
 * label_off / cm, B < 1, D outside 1..1024, nc outside 1..100, a threshold that is < 0 or not finite, a pointer that
 * is not 4-byte aligned. */
int yolosod_confusion_matrix(const float* det, const int* counts, int B, int D, const float* labels,
                             const int* label_off, int nc, float conf_thr, float iou_thr, int32_t* cm, void* stream);
/* ByteTrack per video stream  ultralytics/trackers/byte_tracker.py:293-405 (BYTETracker.update, bytetrack.yaml), from
 * device-resident state, one launch per update and no host sync (csrc/track.hip; the definition is
 * yolo-sod_amd/utils/bytetrack.py). det[b] / counts[b] of every call are the next frame of stream b: padded NMS rows
 * [B][D][6] = x1, y1, x2, y2, conf, cls and their counts (clamped to 0..D); the row index is the track's idx.
 * state: B * yolosod_track_state_bytes(T) bytes, 8-byte aligned, owned by the caller and touched only through these
 * entries: per stream a 64-byte header (int32 frame, next id, overflow), fp64 means [8][T] and covariances [64][T],
 * int32 state / flags / id / start frame / last frame / idx [T] each, fp32 score / cls [T] each (state: 0 free, 1
 * Tracked, 2 Lost, 3 Removed but still listed as lost; flags: 1 activated, 2 the id was removed once).
 * yolosod_track_reset zeroes the state of the n streams listed in streams (device int32, or NULL: all B) and starts
 * their ids at 1; it must run once before the first update. params: HOST float[8] = track_high_thresh,
 * track_low_thresh, new_track_thresh, match_thresh, the second (0.5) and unconfirmed (0.7) association thresholds,
 * max_time_lost (frames), fuse_score (0 / 1); all compared in fp32. tracks: [B][T][8] = x1, y1, x2, y2, track_id,
 * score, cls, idx per activated tracked track, ascending track_id, rows >= n_tracks[b] zero; n_tracks: [B].
 * workspace: yolosod_track_workspace(B, T, D) bytes, 16-byte aligned (per stream the association's boxes and its
 * [T][D] fp32 cost matrix). A birth without a free slot is skipped and counted in the stream's overflow word.
 * Refused before any launch: a null pointer, B < 1, T not a multiple of 64 in 64..1024, D outside 1..1024, a
 * workspace that is too small, a parameter that is < 0 or not finite, a misaligned pointer. */
size_t yolosod_track_state_bytes(int T);
size_t yolosod_track_workspace(int B, int T, int D);
int yolosod_track_reset(void* state, int B, int T, const int* streams, int n, void* stream);
int yolosod_track_update(void* state, int B, int T, const float* det, const int* counts, int D, const float* params,
                         float* tracks, int* n_tracks, void* workspace, size_t ws_bytes, void* stream);
/* BoT-SORT per video stream  ultralytics/trackers/bot_sort.py (BOTSORT, botsort.yaml; ReID is a stub there), the same
 * update with a choice of the filter's model (the definition is yolo-sod_amd/utils/botsort.py):
 * model 0 is XYAH and gives exactly yolosod_track_update; model 1 is XYWH (KalmanFilterXYWH, kalman_filter.py:289-491:
 * state cx, cy, w, h, noise from w and h separately, both size velocities zeroed before a track that is not Tracked is
 * predicted). warps: device double [B][2][3], 8-byte aligned, or NULL: stream b's camera-motion matrix from its previous
 * frame to this one, in the pixels of det; with model 1 every pool and unconfirmed track is warped by it between the
 * prediction and the first association (STrack.multi_gmc, byte_tracker.py:103-120, 332-335). A warp with a non-finite
 * entry is skipped for that stream and counted in the fourth int32 of its header (bad_warp); a finite one is applied
 * as given. State layout, yolosod_track_state_bytes and the workspace are those of yolosod_track_update; a state must
 * stay with one model between resets. Refused before any launch: everything yolosod_track_update refuses, a model
 * other than 0 or 1, warps with model 0, warps that are not 8-byte aligned. */
int yolosod_track_update_ex(void* state, int B, int T, const float* det, const int* counts, int D, const float* params,
                            int model, const double* warps, float* tracks, int* n_tracks, void* workspace,
                            size_t ws_bytes, void* stream);
/* Test hook (host only): facts of this thread's last yolosod_track_update / _ex launch: 0 T, 1 D, 2 B, 3 the workspace
 * layout (1: track boxes [T], detection boxes [D], cost matrix [T][D] per stream), 4 lanes per workgroup, 5 workspace
 * bytes per stream, 6 the model (0 XYAH, 1 XYWH), 7 whether warps were given (0 / 1); 0 before the first launch, -1
 * for another what. */
int yolosod_debug_track_last(int what);

/* Conv epilogue for the PyTorch-ROCm backbone convs (not a reference hot-path op; conv.py:37-55 + block.py:343-356
 * + Concat): out[b*out_bstride + c*HW + p] = act(y[b*y_bstride + c*HW + p] + bias[c]) (+ res[...]); act 0 id, 1 SiLU.
 * Writes into channel slices of a concat buffer via out_bstride; in place allowed. */
int yolosod_bias_act(const float* y, long y_bstride, float* out, long out_bstride, const float* bias,
                     const float* res, long res_bstride, int B, int C, long HW, int act, void* stream);

/* yolosod_bias_act that also stores channels [c2lo, C) of the result packed in out2 ([B, C - c2lo, HW], batch
 * stride out2_bstride): C2f's Bottleneck chain (block.py:249-253, :343-356) reads channel slices of the concat
 * buffer, which MIOpen would otherwise make contiguous with a copy pass per Bottleneck. */
int yolosod_bias_act_dual(const float* y, long y_bstride, float* out, long out_bstride, const float* bias,
                          const float* res, long res_bstride, float* out2, long out2_bstride, int c2lo, int B, int C,
                          long HW, int act, void* stream);

/* Detect head tower conv (ultralytics/nn/modules/head.py:43-57, conv.py:37-55): 3x3 / stride 1 /
 * pad 1 conv with 64 outputs + folded-BN bias + SiLU, fp32 NCHW in and out, as an implicit GEMM on fp16 two-term
 * split MFMA (csrc/conv3x3.hip). Replaces torch.nn.functional.conv2d (MIOpen) + the bias / SiLU epilogue for those
 * convs. Cin a multiple of 32 (<= 2048). The weights [64][Cin][3][3] are prepared once per version into a caller-
 * owned block of yolosod_conv3x3_prep_bytes(Cin) bytes (0: unsupported Cin). */
size_t yolosod_conv3x3_prep_bytes(int cin);
int yolosod_conv3x3_prepare(const float* w, int cin, void* prep, size_t prep_bytes, void* stream);
int yolosod_conv3x3_silu(const float* x, float* y, int B, int cin, int H, int W, const float* bias, const void* prep,
                         size_t prep_bytes, void* stream);
/* General form (the neck's C2f Bottleneck convs too): Cout 32 or a multiple of 64 (<= 512); the output image b at
 * y + b*y_bstride (a concat slice), res (or NULL) added after the activation (Bottleneck shortcut); _xs: the input image
 * b at x + b*x_bstride (a channel slice, e.g. of the C2f's own buffer); _ex: contiguous x. */
size_t yolosod_conv3x3_prep_bytes_ex(int cin, int cout);
int yolosod_conv3x3_prepare_ex(const float* w, int cin, int cout, void* prep, size_t prep_bytes, void* stream);
int yolosod_conv3x3_silu_ex(const float* x, float* y, long y_bstride, const float* res, long res_bstride, int B,
                            int cin, int cout, int H, int W, const float* bias, const void* prep, size_t prep_bytes,
                            void* stream);
int yolosod_conv3x3_silu_xs(const float* x, long x_bstride, float* y, long y_bstride, const float* res, long res_bstride,
                            int B, int cin, int cout, int H, int W, const float* bias, const void* prep,
                            size_t prep_bytes, void* stream);
/* A C2f Bottleneck of 32 channels (Cin = Cmid = Cout = 32: the two P2 C2fs) as one launch:
 * y = [res +] SiLU(conv3x3(SiLU(conv3x3(x, W1) + bias1), W2) + bias2), the intermediate map kept on chip, bit-identical
 * to two yolosod_conv3x3_silu_xs launches. W % 4 == 0 and 16-byte aligned images only (others: error); image b of
 * x / y / res at x + b*x_bstride / y + b*y_bstride / res + b*res_bstride (channel slices of a concat buffer); res NULL:
 * no shortcut; prep1 / prep2: yolosod_conv3x3_prepare_ex(w, 32, 32, ...) of the two convs. y must not alias x / res.
 * The entry always runs the one launch; yolosod_debug_bottleneck3x3_fused says when it is the faster choice. */
int yolosod_bottleneck3x3_silu_xs(const float* x, long x_bstride, float* y, long y_bstride, const float* res,
                                  long res_bstride, int B, int H, int W, const float* bias1, const void* prep1,
                                  size_t prep1_bytes, const float* bias2, const void* prep2, size_t prep2_bytes,
                                  void* stream);

/* A Detect tower's last 3x3 conv (64 -> 64, BN folded, SiLU) with the tower's 1x1 conv and the decode in its epilogue:
 * mode 1 the box tower (64 DFL logits -> rows 0 .. 3 of y: cx, cy, w, h), mode 2 the class tower (nc logits -> rows
 * 4 .. 4 + nc - 1: scores), anchors a_off .. a_off + H*W - 1 of y [B][4 + nc][A]; the other elements of y are not
 * written. The [B][64][H][W] feature map is never stored. Bit-identical to yolosod_conv3x3_silu_xs followed by
 * yolosod_detect_head_levels on that level. prep: yolosod_conv3x3_prepare_ex(w, 64, 64, ...); head_prep:
 * yolosod_detect_head_prepare of the 1x1 weight; head_bias [64] / [nc]. reg_max 16, 1 <= nc <= 16, W % 4 == 0 and
 * 16-byte aligned images (image b at x + b*x_bstride); anything else is an error. The split-range flag reports the
 * staged input, the features and both prepared blocks. The entry always runs the one launch;
 * yolosod_debug_conv3x3_head_fused says when it is the routed choice. */
int yolosod_conv3x3_head_xs(const float* x, long x_bstride, int B, int H, int W, const float* bias, const void* prep,
                            size_t prep_bytes, const void* head_prep, const float* head_bias, int mode, int nc,
                            float stride, float* y, int A, int a_off, void* stream);
/* The prepared block of a tower's last 1x1 conv w [rows][64] (rows 64: box; 1 .. 16: class) for the entry above: the
 * fp16 two-term split of 64 w in the head kernel's [t][s][g][row][i] planes (class rows past `rows` zero) and the
 * block's range word, written once per parameter version. yolosod_detect_head_prep_bytes: its size (0: unsupported). */
size_t yolosod_detect_head_prep_bytes(int rows);
int yolosod_detect_head_prepare(const float* w, int rows, void* prep, size_t prep_bytes, void* stream);

/* Thin fused 1x1 convolution of the backbone (conv.py:37-55 after fuse(), 1x1 case): out = SiLU(W x + bias) (+ res)
 * for Cout in {64, 128}, Cin in {64, 96, 128, 192, 256}, HW % 64 == 0; x / out / res may be channel slices (batch
 * strides, multiples of 4); out2 (optional, NULL) = packed copy of channels [c2lo, Cout). Other shapes: error. */
int yolosod_conv1x1_thin(const float* x, long x_bs, const float* w, const float* bias, float* out, long out_bs,
                         const float* res, long res_bs, float* out2, long out2_bs, int c2lo, int B, int Cin, int Cout,
                         long HW, void* stream);

/* SPPF's pooling pyramid (block.py SPPF: three chained MaxPool2d(5, 1, 2) + torch.cat) in one pass over the concat
 * buffer z [B][4C][H][W] (image b at z + b*z_bstride, images contiguous): channels [C, 4C) <- the 5 / 9 / 13-window max
 * pools (clipped to the image; = the chained pools) of channels [0, C), which cv1 wrote. H*W <= 4096. */
int yolosod_sppf_pool(float* z, long z_bstride, int B, int C, int H, int W, void* stream);

/* yolosod_conv1x1_thin (no res) over a virtual concat [x; x2]: channels [0, k1) from x, [k1, Cin) from x2 (any split);
 * bit-identical to the materialised concat. up_w != 0: x is the quarter-size source [k1][H/2][up_w/2] of a nearest 2x
 * upsample, read in place at (y >> 1, x >> 1); up_w = the output width W (W % 4 == 0, H = HW / W even); bit-identical
 * to the upsampled-and-concatenated input. */
int yolosod_conv1x1_thin_cat(const float* x, long x_bs, const float* x2, long x2_bs, int k1, const float* w,
                             const float* bias, float* out, long out_bs, float* out2, long out2_bs, int c2lo, int B,
                             int Cin, int Cout, long HW, int up_w, void* stream);

/* yolosod_conv1x1_thin (no res / out2) that also emits the output's per-plane statistics for a following SE / CBAM
 * gate in the psum / pmax[B*Cout*parts] layout of yolosod_se_forward_pre / yolosod_cbam_forward_pre (parts =
 * yolosod_plane_parts(HW); plane total in k = 0, 0 / -inf in k > 0); pmax may be NULL; tile_ws = 2*B*Cout*(HW/64)
 * floats of scratch. */
int yolosod_conv1x1_thin_stats(const float* x, long x_bs, const float* w, const float* bias, float* out, long out_bs,
                               int B, int Cin, int Cout, long HW, int parts, float* psum, float* pmax, float* tile_ws,
                               void* stream);

/* 1x1 convolution (stride 1, groups 1) of the backbone as an fp32 MFMA GEMM with the epilogue fused:
 * out[b*out_bs + m*HW + p] = act(sum_k w[m][k] x[b*x_bs + k*HW + p] + bias[m]) (+ res[...]); Cin % 32 == 0. */
int yolosod_conv1x1(const float* x, long x_bs, const float* w, const float* bias, float* out, long out_bs,
                    const float* res, long res_bs, int B, int Cin, int Cout, long HW, int act, void* stream);

/* Building blocks, exported for unit tests (no single reference interface):
 * C(b,m,n) = act(sum_k A(b,m,k) B(b,k,n) + bias) + res;  A K-contiguous; B K- or N-contiguous. */
int yolosod_gemm_f32(const float* A, long a_bs, int lda, const float* B, long b_bs, int ldb, int b_kcontig, float* C,
                     long c_bs, int ldc, int M, int N, int K, int batch, const float* bias, int bias_mode, int act,
                     const float* res, void* stream);
int yolosod_layernorm(const float* x, float* y, long rows, int C, const float* w, const float* b, float eps,
                      void* stream);
int yolosod_attention(const float* qkv, float* out, long n_seq, int L, int C, int heads, void* stream);

/* Test hook: 1 routes SwinBlock shapes the fused per-window kernel covers (C 64/128, heads 2/4, window <= 7x7,
 * mlp 2C) through it (default), 0 forces the decomposed GEMM path for every shape. */
void yolosod_debug_set_swin_fused(int on);
/* Test hook: 1 (default; env YOLOSOD_SWIN_X3=0 turns it off) routes 7x7-window SwinBlocks with C = 64 / 2 heads and
 * C = 256 / 4 heads through the kernels that run every matrix product as fp16 two-term splits on the fp16 matrix
 * cores at fp32 accuracy (csrc/swin_x3.hip), 0 through the exact-fp32-MFMA fused kernels. */
int yolosod_debug_set_swin_x3(int on);
/* Test hooks (host only, no launch): the route of SwinBlock. yolosod_debug_swin_route: the one yolosod_swin_forward
 * takes for this shape under the current switches, from the launchers' own conditions - 0 decomposed GEMM path,
 * 1 fp16-split fused (csrc/swin_x3.hip), 2 exact fused (csrc/swin_fused.hip), 3 exact wide (csrc/swin_wide.hip),
 * -1 a shape it rejects. yolosod_debug_swin_last_route: the one the last yolosod_swin_forward /
 * yolosod_swin_forward_prepared call of this process took (-1: none yet), recorded where the launcher reported its
 * launch. */
int yolosod_debug_swin_route(int B, int C, int num_heads, int H, int W, int window, int mlp_hidden);
int yolosod_debug_swin_last_route(void);
/* The yolosod_debug_set_* switches that return int return the previous state. */
/* Test hook: pixels per area group of the A2 proj + SiLU + pooling kernel (the launcher takes the fewest area groups
 * whose row bands fit; 208 by default - two workgroups per CU; <= 0 restores 208). Same
 * results for every cap. Returns the previous cap. */
int yolosod_debug_set_a2_pool_px(int px);
/* Test hook: 1 (default; env YOLOSOD_HEAD_X2=0 turns it off) runs the Detect head's 1x1 convs as fp16 two-term
 * splits on the fp16 matrix cores (detect_head_x2_kernel), 0 on the exact fp32 MFMA (detect_head_lds_kernel). */
int yolosod_debug_set_head_x2(int on);
/* Test hooks: A2_Attn's GEMMs as fp16 two-term splits on v_mfma_f32_32x32x16_f16 (1, default; env YOLOSOD_A2_X2=0
 * turns it off) or exact fp32 MFMA (0); yolosod_debug_set_gemm_x2(1) makes every yolosod_gemm_f32 / internal fp32 GEMM
 * call take the split products, 0 restores the callers' choice. */
int yolosod_debug_set_a2_x2(int on);
/* Test hook: A2_Attn's split path through the fused kernels (1, default:
 * proj + SiLU + pooling, then LN + QKV + attention, csrc/a2_fused.hip) or the decomposed GEMM path (0). */
int yolosod_debug_set_a2_fused(int on);
/* Test hook: A2_Attn's proj + SiLU + pooling kernel with 128 / 256 output channels per workgroup (1, default)
 * or with 64 (0); returns the previous state. */
int yolosod_debug_set_a2_pool_wide(int on);
/* The SE gate only, sigmoid(fc2(relu(fc1(mean_hw(x)))))   smallobj_modules.py:87-90, into gate [B][C], for a consumer
 * that applies y = x * gate itself (yolosod_conv3x3s2_silu); psum: x's per-plane partial sums from its producer
 * (yolosod_bias_act_stats) or NULL (a statistics pass over x). workspace: yolosod_se_workspace bytes. */
int yolosod_se_gate(const float* x, int B, int C, int H, int W, const float* fc1_w, const float* fc1_b,
                    const float* fc2_w, const float* fc2_b, int hidden, const float* psum, float* gate, void* workspace,
                    size_t workspace_bytes, void* stream);
/* The CBAM gates only   cbam_block.py:14-23,33-37: ca [B][C] and sa [B][H][W] (sa from the channel statistics of
 * x * ca), for a consumer that applies y = (x * ca) * sa itself; psum / pmax from the producer or both NULL.
 * workspace: yolosod_cbam_workspace bytes. */
int yolosod_cbam_gates(const float* x, int B, int C, int H, int W, const float* fc0_w, const float* fc2_w, int hidden,
                       const float* sa_w, const float* psum, const float* pmax, float* ca, float* sa, void* workspace,
                       size_t workspace_bytes, void* stream);
/* 3x3 / stride 2 / pad 1 conv + bias + SiLU with the producing MAFN gate applied while the input is staged
 * (csrc/conv3x3s2.hip): y = SiLU(conv3x3_s2((x * gc) * gp, W) + bias), the consumer Conv of SE_Block L1 (gc = the SE
 * gate, smallobj_modules.py:92) and of CBAM_Block L4 (gc = ca, gp = sa, cbam_block.py:53-54) in the paper YAML, with the
 * gate's output never written. fp16 two-term split MFMA at fp32 accuracy; Cout 64 or 128 (_out: multiples of 128 up to
 * 512 too), Cin a multiple of 32 (<= 2048),
 * Ho = (H + 1) / 2, Wo = (W + 1) / 2 with Wo % 4 == 0; x [B][cin][H][W] (B*cin*H*W*4 < 2^32), gc [B][cin] 16-byte
 * aligned or NULL, gp [B][H][W] or NULL, y [B][cout][Ho][Wo]. Weights prepared once per parameter version into a
 * caller-owned block of yolosod_conv3x3s2_prep_bytes(cin, cout) bytes (0: unsupported). Replaces the gate's apply pass
 * + torch.nn.functional.conv2d (MIOpen) + the bias / SiLU epilogue. */
size_t yolosod_conv3x3s2_prep_bytes(int cin, int cout);
int yolosod_conv3x3s2_prepare(const float* w, int cin, int cout, void* prep, size_t prep_bytes, void* stream);
int yolosod_conv3x3s2_silu(const float* x, float* y, int B, int cin, int cout, int H, int W, const float* bias,
                           const float* gc, const float* gp, const void* prep, size_t prep_bytes, void* stream);
/* The same with image b's output [cout][Ho][Wo] at y + b * y_bstride (y_bstride >= cout*Ho*Wo, a multiple of 4, y
 * 16-byte aligned): a channel slice of a concat buffer (nn/tasks.py concat elision). Cout may also be any multiple of
 * 128 up to 512 (the PAN neck's stride-2 convs, layers 29 / 33 / 36 of the paper YAML). */
int yolosod_conv3x3s2_silu_out(const float* x, float* y, long y_bstride, int B, int cin, int cout, int H, int W,
                               const float* bias, const float* gc, const float* gp, const void* prep,
                               size_t prep_bytes, void* stream);
/* 1x1 / stride 1 conv + bias + SiLU on the fp16 two-term split MFMA at fp32 accuracy (csrc/conv1x1x2.hip): the PAN
 * neck's wide 1x1 convs (C2f cv1 / cv2, lateral convs; conv.py:37-55, block.py:249-253). Cout a multiple of 128 (<= 1024),
 * Cin a multiple of 32 (<= 4096, weights padded to 128), HW % 4 == 0. x image b at x + b*x_bstride ([cin][HW]); y image
 * b at y + b*y_bstride ([cout][HW], a concat slice when the stride is larger); y2 (or NULL): channels [c2lo, cout)
 * stored again at y2 + b*y2_bstride (C2f's first Bottleneck input). Replaces MIOpen's fp32 GEMM + the bias / SiLU pass. */
size_t yolosod_conv1x1x2_prep_bytes(int cin, int cout);
int yolosod_conv1x1x2_prepare(const float* w, int cin, int cout, void* prep, size_t prep_bytes, void* stream);
int yolosod_conv1x1x2_silu(const float* x, long x_bstride, float* y, long y_bstride, float* y2, long y2_bstride,
                           int c2lo, int B, int cin, int cout, int HW, const float* bias, const void* prep,
                           size_t prep_bytes, void* stream);
/* The same over a virtual concat [x; x2] (block.py:249-253: the C2f cv1 after a neck Concat): channels [0, k1) from x
 * (image b at x + b*x_bstride), [k1, cin) from x2 (image b at x2 + b*x2_bstride), k1 a multiple of 128; x2 NULL:
 * yolosod_conv1x1x2_silu. Bit-identical to the materialised concat. up_w != 0 (needs x2): x is the quarter-size source
 * [k1][H/2][up_w/2] of a nearest 2x upsample, read in place at (y >> 1, x >> 1); up_w = the output width W (W and
 * H = HW / W even); bit-identical to the upsampled-and-concatenated input. */
int yolosod_conv1x1x2_silu_cat(const float* x, long x_bstride, const float* x2, long x2_bstride, int k1, float* y,
                               long y_bstride, float* y2, long y2_bstride, int c2lo, int B, int cin, int cout, int HW,
                               const float* bias, const void* prep, size_t prep_bytes, int up_w, void* stream);
/* yolosod_conv1x1x2_silu (one input, no y2) that also emits y's per-plane statistics for the SE (stats 1: sums) / CBAM
 * (stats 2: sums and maxes, pmax required) gate that follows, from the values as its epilogue stores them: psum /
 * pmax[B*cout*parts] in the layout of yolosod_se_forward_pre / yolosod_cbam_forward_pre (parts =
 * yolosod_plane_parts(HW); k = 0 holds the plane's total, k > 0 hold 0 / -inf). tile_ws: 2*B*cout*ceil(HW/64) floats.
 * No atomics: deterministic, independent of B. y is bit-identical to yolosod_conv1x1x2_silu's. The forced group field
 * of yolosod_debug_set_conv1x1x2_form holds; the statistics forms have one pair of staged planes. */
int yolosod_conv1x1x2_silu_stats(const float* x, long x_bstride, float* y, long y_bstride, int B, int cin, int cout,
                                 int HW, const float* bias, const void* prep, size_t prep_bytes, int stats, int parts,
                                 float* psum, float* pmax, float* tile_ws, void* stream);
/* Test / measurement hook: force the form of the fp16-split 1x1 conv kernel (csrc/conv1x1x2.hip); every form gives
 * bit-identical results. form = groups + 4 * buffers. groups: 0 automatic, 1 workgroups of 128 output channels (two
 * 16-channel blocks per wave), 2 of 256 (four blocks per wave; Cout % 256 == 0, any other Cout runs groups 1).
 * buffers: 0 automatic, 1 one pair of staged fp16 planes (two barriers per stage), 2 two pairs (double-buffered: one
 * barrier per stage, 69632 B of LDS). Cout 64 has one form, reported as 1 + 4 * 1. Values outside [0, 12) and groups
 * 3 are ignored. Returns the previous value. */
int yolosod_debug_set_conv1x1x2_form(int form);
/* The form (same encoding, no field 0) a [B][*][H][W] -> cout launch of yolosod_conv1x1x2_silu* runs in under the
 * current setting; 0 for shapes the kernel does not take (H * W not a multiple of 4, unsupported cout). */
int yolosod_debug_conv1x1x2_form(int B, int cout, int H, int W);
/* Test / measurement hook: the form the tiled stride-2 conv kernel (csrc/conv3x3s2.hip) takes. form = geometry +
 * 4 * groups: geometry 0 automatic, 1 the 32 x 2 output tile of 16 x 1 pixel blocks, 2 the 40 x 2 tile of 8 x 2 blocks,
 * 3 the 20 x 4 tile of 4 x 4 blocks; groups 0 automatic, 1 128-channel output groups, 2 64-channel groups (Cout 64 always
 * runs 64-channel groups). Every form gives bit-identical results. Values outside [0, 12) are ignored. Returns the
 * previous value. */
int yolosod_debug_set_conv3x3s2_form(int form);
/* The form (same encoding, no field 0) a [B][*][H][W] -> cout launch of yolosod_conv3x3s2_silu* runs in under the
 * current setting; 0 for shapes the kernel does not take (output width not a multiple of 4, unsupported cout). */
int yolosod_debug_conv3x3s2_form(int B, int cout, int H, int W);
/* Test / measurement hook: force the form of the persistent 3x3 conv kernel (csrc/conv3x3.hip, W % 4 == 0 shapes);
 * every form gives bit-identical results. form = geometry + 4 * groups. geometry: 0 automatic (the fewest tiles for
 * the map), 1 the 32 x 8 tile of 16 x 1 blocks, 2 the 20 x 12 tile of 4 x 4 blocks, 3 the 40 x 6 tile of 8 x 2
 * blocks. groups: 0 automatic (32-channel groups when 64-channel work items would leave workgroup slots idle), 1
 * 64-channel output groups (an error for Cout 32), 2 32-channel groups, 3 the 32-channel group with the wave's whole
 * weight set resident in registers (Cin 32 -> Cout 32; any other shape runs groups 2), 4 the 32-channel group with
 * both 16-channel blocks on every wave (Cout 32; any other Cout runs groups 2). Values outside [0, 20) are ignored.
 * Returns the previous value. */
int yolosod_debug_set_conv3x3_form(int form);
/* The form (same encoding, no field 0) a [B][*][H][W] -> cout launch of yolosod_conv3x3_silu* runs in under the current
 * setting; 0 for shapes the persistent kernel does not take (W % 4 != 0, unsupported cout). */
int yolosod_debug_conv3x3_form(int B, int cout, int H, int W);
/* As yolosod_debug_conv3x3_form for a known Cin: groups 3 / 4 are chosen (automatically, or forced) for Cin 32 ->
 * Cout 32 only, and yolosod_debug_conv3x3_form answers for every other Cin. */
int yolosod_debug_conv3x3_form_ex(int B, int cin, int cout, int H, int W);
/* Whether a [B][32][H][W] Bottleneck is to run as yolosod_bottleneck3x3_silu_xs (1) or as the two conv launches (0)
 * under the current setting: automatically, from a map size (B*32*H*W*4 bytes) at which the pair's intermediate no
 * longer stays in cache between its launches; never for W % 4 != 0. Host-side, no GPU needed. */
int yolosod_debug_bottleneck3x3_fused(int B, int H, int W);
/* Test / measurement hook for the answer above: -1 automatic (default), 0 never, 1 every shape the kernel takes.
 * Other values are ignored. Returns the previous value. */
int yolosod_debug_set_bottleneck3x3_fuse(int mode);
/* Whether a Detect level with [B][64][H][W] tower maps is to run its towers' last convs as yolosod_conv3x3_head_xs (1)
 * or as conv launches followed by the head kernel (0) under the current setting: automatically, when the 64 -> 64
 * launch of that shape runs in 64-channel groups (yolosod_debug_conv3x3_form); never for W % 4 != 0. Host-side. */
int yolosod_debug_conv3x3_head_fused(int B, int H, int W);
/* Test / measurement hook for the answer above: -1 automatic (default), 0 never, 1 every shape the kernel takes.
 * Other values are ignored. Returns the previous value. */
int yolosod_debug_set_conv3x3_head_fuse(int mode);
void yolosod_debug_set_gemm_x2(int on);
/* Test hook: the bf16 decomposed SwinBlock's depthwise conv + token layout and LN1 in one pass
 * (swin_tokens_ln_bf16_kernel, 1, default) or as two kernels (0);
 * bit-identical. Returns the previous state. */
int yolosod_debug_set_swin_tokln(int on);
/* Test hook: the fp16 two-term split of the fp32-accurate matrix kernels (common.h split2) on npair pairs of v:
 * h[i] = the fp16 pair (fp16(v[2i]), fp16(v[2i+1])), l[i] = (fp16(v[2i] - h.lo), fp16(v[2i+1] - h.hi)), as 2 x 16-bit
 * patterns per uint32 (low half = even element). Device pointers. */
int yolosod_debug_split_f16(const float* v, uint32_t* h, uint32_t* l, long npair, void* stream);
/* Split-range guard of the fp32-accurate fp16-split kernels (Swin x3 / wx and their weight preparation, Detect head
 * x2, the X2 GEMMs): fp16 represents |v| < 65520 only, so every split site records the largest magnitude it split and
 * a kernel that saw one beyond 65504 (or a NaN) sets the current device's flag word. Returns 1 if set since the last
 * reset, 0 if not, < 0 on error; synchronises `stream` first; reset != 0 clears it. A caller that sees 1 redoes the
 * work on the exact-fp32-MFMA kernels (the yolosod_debug_set_*(0) switches; DetectionPredictor does). */
int yolosod_split_range_flag(int reset, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * bf16 model config (BASELINE configs[4]): `model.to(torch.bfloat16)` after fuse() - AutoBackend's fp16
 * route (autobackend.py:145-156, predictor im.half()) with bfloat16. Activations (x, y, res, out2, tower features)
 * and the GEMM weights of Swin / A2 are bf16 bit patterns (uint16_t, torch.bfloat16 layout); every other parameter,
 * the statistics / partials and Detect's output are fp32. Arithmetic is fp32 (bf16 MFMA with fp32 accumulation for
 * the GEMMs and attention); each stored tensor is rounded once (nearest even). Same argument meaning and workspace
 * queries as the fp32 entry points above unless noted.
 * ------------------------------------------------------------------------------------------------------------- */
#include <stdint.h>

/* SE (smallobj_modules.py:84-92); psum = producer partials (yolosod_bias_act_stats_bf16) or NULL. */
int yolosod_se_forward_bf16(const uint16_t* x, uint16_t* y, int B, int C, int H, int W, const float* fc1_w,
                            const float* fc1_b, const float* fc2_w, const float* fc2_b, int hidden, const float* psum,
                            void* workspace, size_t workspace_bytes, void* stream);
/* CBAM (cbam_block.py:52-55); psum / pmax both NULL or both the producer's partials. */
int yolosod_cbam_forward_bf16(const uint16_t* x, uint16_t* y, int B, int C, int H, int W, const float* fc0_w,
                              const float* fc2_w, int hidden, const float* sa_w, const float* psum, const float* pmax,
                              void* workspace, size_t workspace_bytes, void* stream);
/* CA (ca_block.py:38-59); yin = producer's pooled means (yolosod_bias_act_capool_bf16) or NULL. */
int yolosod_ca_forward_bf16(const uint16_t* x, uint16_t* y, int B, int C, int H, int W, const float* conv1_w,
                            const float* conv1_b, int mip, const float* bn_w, const float* bn_b, const float* bn_mean,
                            const float* bn_var, float bn_eps, const float* convh_w, const float* convh_b,
                            const float* convw_w, const float* convw_b, const float* yin, void* workspace,
                            size_t workspace_bytes, void* stream);
/* SwinBlock.forward (blocks_transformer.py:150-171): in_proj_w [3C][C], out_proj_w [C][C], mlp1_w [hid][C],
 * mlp2_w [C][hid], pw_w [C][C] bf16; C % 64 == 0, head dim 32 / 64 / 128. */
size_t yolosod_swin_workspace_bf16(int B, int C, int H, int W, int num_heads, int window, int mlp_hidden);
int yolosod_swin_forward_bf16(const uint16_t* x, uint16_t* y, int B, int C, int H, int W, int num_heads, int window,
                              const float* dw_w, const float* ln1_w, const float* ln1_b, float ln1_eps,
                              const uint16_t* in_proj_w, const float* in_proj_b, const uint16_t* out_proj_w,
                              const float* out_proj_b, const float* ln2_w, const float* ln2_b, float ln2_eps,
                              const uint16_t* mlp1_w, const float* mlp1_b, int mlp_hidden, const uint16_t* mlp2_w,
                              const float* mlp2_b, const uint16_t* pw_w, const float* bn_w, const float* bn_b,
                              const float* bn_mean, const float* bn_var, float bn_eps, void* workspace,
                              size_t workspace_bytes, void* stream);
/* A2_Attn.forward (a2_attn.py:35-69), residual form, pre-multiplied output weights (oproj_w = Wconv . Wmha,
 * oproj_b = Wconv . bmha + bconv); proj_w / in_proj_w / oproj_w bf16; head dim 32 / 64 / 128, H*W % 8 == 0. */
size_t yolosod_a2_workspace_bf16(int B, int C, int H, int W, int num_areas);
int yolosod_a2_forward_bf16(const uint16_t* x, uint16_t* y, int B, int C, int H, int W, int num_areas, int num_heads,
                            const uint16_t* proj_w, const float* proj_b, const float* ln_w, const float* ln_b,
                            float ln_eps, const uint16_t* in_proj_w, const float* in_proj_b, const uint16_t* oproj_w,
                            const float* oproj_b, void* workspace, size_t workspace_bytes, void* stream);
/* Detect head tail + decode (as yolosod_detect_head) of levels [l0, l1) only, into y laid out for all nl levels
 * (the anchor offsets and A of every level; the other levels' slices of y are not written and their feature
 * pointers not read). bf16 != 0: bf16 tower features (uint16_t patterns). Lets a caller decode the levels whose
 * tower convolutions are done while the last level's still run (head.py:70 per level + _inference :100-131). */
int yolosod_detect_head_levels(int nl, int l0, int l1, const void* const* box_feat, const void* const* cls_feat, int c2,
                               int c3, const float* const* box_w, const float* const* box_b, const float* const* cls_w,
                               const float* const* cls_b, const int* heights, const int* widths, const float* strides,
                               int B, int nc, int reg_max, float* y, int bf16, void* stream);
/* Detect head tail + decode (as yolosod_detect_head) on bf16 tower features; weights, biases and y fp32. */
int yolosod_detect_head_bf16(int nl, const uint16_t* const* box_feat, const uint16_t* const* cls_feat, int c2, int c3,
                             const float* const* box_w, const float* const* box_b, const float* const* cls_w,
                             const float* const* cls_b, const int* heights, const int* widths, const float* strides,
                             int B, int nc, int reg_max, float* y, void* stream);
/* Conv epilogues on bf16 maps (yolosod_bias_act / _dual / _stats / _capool); out2 NULL = no second store. The
 * statistics are fp32 sums / maxes / means of the stored (rounded) values. */
int yolosod_bias_act_bf16(const uint16_t* y, long y_bstride, uint16_t* out, long out_bstride, const float* bias,
                          const uint16_t* res, long res_bstride, uint16_t* out2, long out2_bstride, int c2lo, int B,
                          int C, long HW, int act, void* stream);
int yolosod_bias_act_stats_bf16(const uint16_t* y, long y_bstride, uint16_t* out, long out_bstride, const float* bias,
                                const uint16_t* res, long res_bstride, int B, int C, long HW, int act, int parts,
                                long seg, float* psum, float* pmax, void* stream);
int yolosod_bias_act_capool_bf16(const uint16_t* y, long y_bstride, uint16_t* out, long out_bstride,
                                 const float* bias, const uint16_t* res, long res_bstride, int B, int C, int H, int W,
                                 int act, float* yin, void* stream);
/* Test hooks: bf16 GEMM (bf16 out, fp32 accumulation; K % 64 == 0) and attention over contiguous sequences. */
int yolosod_gemm_bf16(const uint16_t* A, long a_bs, int lda, const uint16_t* B, long b_bs, int ldb, int b_kcontig,
                      uint16_t* C, long c_bs, int ldc, int M, int N, int K, int batch, const float* bias,
                      int bias_mode, int act, const uint16_t* res, void* stream);
int yolosod_attention_bf16(const uint16_t* qkv, uint16_t* out, long n_seq, int L, int C, int heads, void* stream);
/* Report hooks of the bf16 kernels (host only, no launch). Each prediction is answered by the predicate the launcher
 * itself calls; each last_* twin is written where the launch happens, from the launched instance's own constants.
 *  - yolosod_debug_gemm_bf16_tile: the N extent of the bf16 GEMM's workgroup tile for (M, N, batch): 64 (128x64) or 128
 *    (128x128). _last_tile: of the last bf16 GEMM launch of this process (-1: none yet). _launches(tile): how many
 *    launches took that tile so far (-1 for a tile other than 64 / 128).
 *  - yolosod_debug_swin_bf16_route: what yolosod_swin_forward_bf16 runs for this shape under the current switches:
 *    0 decomposed with the two-kernel token path, 1 decomposed with the tokens + LN1 pass, 2 fused per-window kernel
 *    with the 2-byte halo layout, 3 fused with the 16-byte chunk layout, -1 a shape it refuses. _last_route: of the
 *    last yolosod_swin_forward_bf16 call (-1: none yet).
 *  - yolosod_debug_attention_bf16_form: head dim * 100 + key blocks (of 16) of the window_attn_bf16_kernel instance
 *    that takes sequences of L tokens, or -1 for a refused shape. _last_form: of the last bf16 attention launch. */
int yolosod_debug_gemm_bf16_tile(int M, int N, int batch);
int yolosod_debug_gemm_bf16_last_tile(void);
long yolosod_debug_gemm_bf16_launches(int tile);
int yolosod_debug_swin_bf16_route(int B, int C, int num_heads, int H, int W, int window, int mlp_hidden);
int yolosod_debug_swin_bf16_last_route(void);
int yolosod_debug_attention_bf16_form(int L, int C, int heads);
int yolosod_debug_attention_bf16_last_form(void);

#ifdef __cplusplus
}
#endif
#endif /* YOLOSOD_HIP_H */
