/*
 * ovis_hip.h -- C ABI of libovis_hip.so, the MI355X (gfx950) native-op library behind
 * the `maskrcnn_benchmark._C` operator surface of hbdat/cvpr22_cross_modal_pseudo_labeling.
 *
 * Conventions (every entry point):
 *   - plain C linkage, raw DEVICE pointers + explicit sizes, no torch / ATen types;
 *   - tensors are dense, contiguous, row-major (NCHW for feature maps);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is
 *     enqueued asynchronously on it, nothing here synchronises the host unless stated;
 *   - return value: OVIS_OK (0) on success, a negative OVIS_E* code for an argument
 *     error detected on the host, or a positive hipError_t if a HIP call failed.
 *     Nothing throws across this boundary.
 *
 * Each declaration cites the reference interface (path:line under the reference repo,
 * `mb/` = maskrcnn_benchmark/) whose behaviour it reproduces.
 */
#ifndef OVIS_HIP_H_
#define OVIS_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OVIS_OK 0
#define OVIS_EINVAL (-1)    /* bad size / null pointer                     */
#define OVIS_ENOSPC (-2)    /* caller workspace too small                  */
#define OVIS_ERANGE (-3)    /* problem exceeds what the kernel supports    */

/* Library / build identification.  Returns a static NUL-terminated string
 * "ovis_hip <version> gfx950 flags: <the compiler flags of every object>".  The kernel sources have no compile-time
 * switch and a product build carries no -D; experiment variants live in their own libraries
 * (tools/experiments/build_variants.sh). */
const char* ovis_version(void);

/* ------------------------------------------------------------------------------------
 * RoIAlign                                   mb/csrc/ROIAlign.h:11-46
 *   forward : mb/csrc/cuda/ROIAlign_cuda.cu:65-122,257-299 (= cpu/ROIAlign_cpu.cpp:114-219)
 *   backward: mb/csrc/cuda/ROIAlign_cuda.cu:178-254,302-346
 * input  [batch, channels, height, width] f32
 * rois   [num_rois, 5] f32 = (batch_index, x1, y1, x2, y2) in image pixels
 * output [num_rois, channels, pooled_h, pooled_w] f32
 * sampling_ratio <= 0 selects the adaptive grid ceil(roi_size / pooled_size).
 * The forward follows the reference's operation order with FP contraction disabled, so
 * it is bit-identical to the reference CPU kernel on finite inputs.
 * ---------------------------------------------------------------------------------- */
int ovis_roi_align_forward_f32(const float* input, const float* rois, float* output,
                               int num_rois, int batch, int channels, int height,
                               int width, int pooled_h, int pooled_w,
                               float spatial_scale, int sampling_ratio, void* stream);

/* Workspace form of the forward (the fast path).  When
 * ovis_roi_align_forward_mfma_supported(height, width, pooled_h, pooled_w) is non-zero (map
 * at least 16 x 16, pooled sizes at most 16 x 16) the pooled tile of every (RoI, channel)
 * is computed as two 16 x 16 x 16 products on the bf16 matrix pipe with the operands split
 * into bf16 hi + lo parts: same values as the reference up to ~1e-5 relative to sum |w x|
 * (NOT bit-identical; ovis_roi_align_forward_f32 stays the bit-exact kernel).  `workspace`:
 * at least ovis_roi_align_forward_workspace_bytes(num_rois, height, width) bytes of device
 * scratch, 256-byte aligned (per-RoI weight tables, rebuilt by every call).  Unsupported
 * shapes run the exact kernel and ignore the workspace.
 * Replaces ROIAlign_forward_cuda, mb/csrc/cuda/ROIAlign_cuda.cu:257-299. */
size_t ovis_roi_align_forward_workspace_bytes(int num_rois, int height, int width);
int ovis_roi_align_forward_mfma_supported(int height, int width, int pooled_h, int pooled_w);
int ovis_roi_align_forward_ws_f32(const float* input, const float* rois, float* output,
                                  int num_rois, int batch, int channels, int height, int width,
                                  int pooled_h, int pooled_w, float spatial_scale,
                                  int sampling_ratio, void* workspace, size_t workspace_bytes,
                                  void* stream);

/* Forward fused with the consumer's stride (extension): pools only bins (bin_stride*i, bin_stride*j) of a feature map
 * given in NHWC memory ([batch, height, width, channels] contiguous: what the trunk of this library computes in; other
 * layouts are copied to it by the caller).  The res5 head's first 1x1 convolution has stride 2
 * (mb/modeling/backbone/resnet.py:258-275, STRIDE_IN_1X1), so it never reads the other three quarters of the 14x14
 * tile.  Per-bin arithmetic is ovis_roi_align_forward_f32's, samples visited in the reference's order: out[r,i,j,c] is
 * bit-identical to that kernel's [r,c,bin_stride*i,bin_stride*j] on the same map in NCHW.  With oh, ow =
 * ceil(pooled / bin_stride):
 *   pair_out == 0: output [num_rois, oh, ow, channels] fp32 (NHWC); channels % 4 == 0.
 *   pair_out != 0: the same bins in PAIR layout (see ovis_split_pair_f32 below: per 32 channels 64 B bf16 hi | 64 B bf16
 *                  lo, the exact split of the fp32 results), [num_rois * oh * ow, channels] pair rows: the operand of the
 *                  res5 head's first split GEMM without an fp32 copy and a split pass; channels % 32 == 0.
 * input_nhwc and output must be 16-byte aligned.  OVIS_ERANGE when a channel or alignment constraint is not met. */
int ovis_roi_align_forward_strided_from_nhwc_f32(const float* input_nhwc, const float* rois, void* output, int num_rois,
                                                 int batch, int channels, int height, int width, int pooled_h,
                                                 int pooled_w, int bin_stride, float spatial_scale, int sampling_ratio,
                                                 int pair_out, void* stream);

/* grad_input [batch, channels, height, width] is fully overwritten (zero-filled, then
 * accumulated into) by this call; the caller does not need to clear it. */
int ovis_roi_align_backward_f32(const float* grad_output, const float* rois,
                                float* grad_input, int num_rois, int batch,
                                int channels, int height, int width, int pooled_h,
                                int pooled_w, float spatial_scale, int sampling_ratio,
                                void* stream);

/* Workspace form of the backward (the fast path).  When
 * ovis_roi_align_backward_plane_supported(height, width, pooled_h, pooled_w) is non-zero
 * (pooled sizes <= 16 and an H x W f32 plane of at most 40 KB, e.g. the 50 x 84 C4 map) the
 * gradient is computed by the plane-owner matrix-core kernel: one wave owns one
 * (image, channel) plane in LDS, no atomics, no zero-fill pass, bit-reproducible run to
 * run, HBM traffic == grad_output once + grad_input once.  `workspace` is device scratch of
 * at least ovis_roi_align_backward_workspace_bytes(num_rois, batch, height, width) bytes,
 * 256-byte aligned (per-RoI separable weight tables + per-image RoI lists, rebuilt by every
 * call).  Unsupported shapes take the same path as ovis_roi_align_backward_f32 and ignore
 * the workspace.  Replaces ROIAlign_backward_cuda, mb/csrc/cuda/ROIAlign_cuda.cu:302-346. */
size_t ovis_roi_align_backward_workspace_bytes(int num_rois, int batch, int height, int width);
int ovis_roi_align_backward_plane_supported(int height, int width, int pooled_h, int pooled_w);
int ovis_roi_align_backward_ws_f32(const float* grad_output, const float* rois,
                                   float* grad_input, int num_rois, int batch, int channels,
                                   int height, int width, int pooled_h, int pooled_w,
                                   float spatial_scale, int sampling_ratio, void* workspace,
                                   size_t workspace_bytes, void* stream);
/* Backward of ovis_roi_align_forward_strided_from_nhwc_f32 (the pooler fused with the stride of the res5 head's first
 * convolution): grad_output [num_rois, channels, ceil(pooled_h / bin_stride), ceil(pooled_w / bin_stride)] holds the
 * gradient of the bins (bin_stride * i, bin_stride * j) only -- the other bins were never computed, their gradient is
 * zero -- so a quarter of the bytes of the full tile are read at bin_stride 2.  Same workspace as the form above.
 * Plane-owner kernel only: OVIS_ERANGE for shapes it does not cover (scatter into a full tile and use the form above). */
int ovis_roi_align_backward_strided_ws_f32(const float* grad_output, const float* rois, float* grad_input,
                                           int num_rois, int batch, int channels, int height, int width,
                                           int pooled_h, int pooled_w, int bin_stride, float spatial_scale,
                                           int sampling_ratio, void* workspace, size_t workspace_bytes, void* stream);

/* The same backward from the gradient as the producing data-gradient GEMM leaves it: NHWC
 * [num_rois, th, tw, channels] fp32 with th, tw = ceil(pooled / bin_stride) <= 8 (the 7 x 7 tiles of the res5 head;
 * mb/csrc/cuda/ROIAlign_cuda.cu:178-254 restricted to the computed bins).  The layout change the plane-owner kernel
 * needs hands every value over already split into bf16 hi | lo (one 256-byte tile per RoI and channel, kept behind the
 * plan tables in `workspace`): no separate permute copy, no hi/lo arithmetic on the gradient operand per item and
 * channel, two matrix instructions per stage.  OVIS_ERANGE for shapes it does not cover. */
size_t ovis_roi_align_backward_strided_nhwc_workspace_bytes(int num_rois, int batch, int channels, int height, int width);
int ovis_roi_align_backward_strided_nhwc_ws_f32(const float* grad_output_nhwc, const float* rois, float* grad_input,
                                                int num_rois, int batch, int channels, int height, int width,
                                                int pooled_h, int pooled_w, int bin_stride, float spatial_scale,
                                                int sampling_ratio, void* workspace, size_t workspace_bytes,
                                                void* stream);

/* ------------------------------------------------------------------------------------
 * NMS                                        mb/csrc/nms.h:10-28, mb/csrc/cuda/nms.cu:13-131
 * boxes [K,4] f32 xyxy (+1 pixel area convention), scores [K] f32.
 * Greedy suppression in descending-score order (ties: lower index first) with the
 * CUDA comparison `IoU > threshold` (nms.cu:60); set `ge_mode` != 0 for the CPU
 * kernel's `>=` (cpu/nms_cpu.cpp:60).  Survivors are written to keep_out[0..n) as
 * ASCENDING original indices (int64) and n to *num_keep (device int32), entirely on the
 * device: no host round trip of the suppression mask.
 * `workspace` is caller-provided device scratch of at least
 * ovis_nms_workspace_bytes(K) bytes (256-byte aligned).  K above OVIS_NMS_MAX_CANDIDATES: OVIS_ERANGE.
 * ---------------------------------------------------------------------------------- */
#define OVIS_NMS_MAX_CANDIDATES 131072
size_t ovis_nms_workspace_bytes(int num_boxes);
int ovis_nms_f32(const float* boxes, const float* scores, int num_boxes, float threshold,
                 int ge_mode, void* workspace, size_t workspace_bytes, int64_t* keep_out,
                 int32_t* num_keep, void* stream);
/* Grouped form: `groups` [K] int32; a box only suppresses boxes of its own group.  One launch replaces the
 * per-class loop of the detection post-processing (mb/modeling/roi_heads/box_head/inference.py:121-163:
 * `for j in range(1, num_classes): boxlist_nms(boxes of class j)`) -- same survivors as running ovis_nms_f32
 * on every group separately, returned as ascending indices into the K candidates. */
int ovis_nms_grouped_f32(const float* boxes, const float* scores, const int32_t* groups, int num_boxes,
                         float threshold, int ge_mode, void* workspace, size_t workspace_bytes,
                         int64_t* keep_out, int32_t* num_keep, void* stream);

/* Batched, score-sorted form for the RPN proposal pipeline (mb/modeling/rpn/inference.py:95-116,
 * mb/structures/boxlist_ops.py:9-49): boxes [num_images, K, 4] are each image's candidates in DESCENDING score order
 * (the top-k prefix: no sort happens here); `drop` [num_images, K] int32 or NULL: a negative entry marks a box the
 * small-box filter removed in front of the NMS -- it suppresses nothing and never survives.  Per image: survivors as
 * ascending indices (= ascending rank) in keep_out[image, 0..n), zero-filled behind them; num_keep[image] = {n, number
 * of survivors with index < `below`} (those form a prefix of keep_out: the NMS result of the first `below` candidates
 * alone, i.e. of a selector with a smaller pre-NMS top-n).  One mask launch + one reduce launch for the whole batch. */
size_t ovis_nms_presorted_workspace_bytes(int num_images, int num_boxes);
int ovis_nms_presorted_batched_f32(const float* boxes, const int32_t* drop, int num_images, int num_boxes,
                                   float threshold, int ge_mode, int below, void* workspace, size_t workspace_bytes,
                                   int64_t* keep_out, int32_t* num_keep, void* stream);

/* ------------------------------------------------------------------------------------
 * Sorted top-k of the RPN scores             mb/modeling/rpn/inference.py:95
 *   (`objectness.topk(pre_nms_top_n, dim=1, sorted=True)` on the sigmoid scores of the batch)
 * scores [num_rows, row_len] (row stride row_stride, in floats) -> out_scores / out_idx [num_rows, k]: the k largest
 * entries of every row in DESCENDING order and their positions in the row; equal scores come in ascending position
 * (torch.topk leaves the order of ties open).  One key-building launch, one device radix sort of the whole batch
 * (rocPRIM), one emitting launch.  num_rows <= 65535, num_rows * row_len < 2^31.
 * ---------------------------------------------------------------------------------- */
size_t ovis_topk_sorted_workspace_bytes(int num_rows, int row_len);
int ovis_topk_sorted_f32(const float* scores, long row_stride, int num_rows, int row_len, int k, float* out_scores,
                         int64_t* out_idx, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * RPN proposal decode                        mb/modeling/rpn/inference.py:95-114,
 *   mb/modeling/box_coder.py:49-95, mb/structures/bounding_box.py:214-225, mb/structures/boxlist_ops.py:34-49
 * For every image and every candidate k < num_candidates: anchor index topk_idx[image, k] = (y * feature_width + x) *
 * anchors_per_position + a; its regression deltas are box_regression[image * stride_image + (y * feature_width + x) *
 * stride_position + (4 * a + c) * stride_channel] (NCHW [N, 4A, H, W]: strides (4A*H*W, 1, H*W); NHWC rows of a GEMM:
 * (H*W*ld, ld, 1)); its anchor is cell_anchors[a] + (x, y, x, y) * anchor_stride.  Writes the decoded box, clipped to
 * the image (image_wh [num_images, 2] = width, height), to boxes[image, k] and drop[image, k] = 0, or -1 when the
 * clipped box is narrower / lower than min_size.  One launch for the batch.
 * ---------------------------------------------------------------------------------- */
int ovis_rpn_decode_f32(const float* box_regression, long reg_stride_image, long reg_stride_position,
                        long reg_stride_channel, const int64_t* topk_idx, const float* cell_anchors,
                        const float* image_wh, int num_images, int num_candidates, int anchors_per_position,
                        int feature_width, float anchor_stride, float weight_x, float weight_y, float weight_w,
                        float weight_h, float xform_clip, float min_size, float* boxes, int32_t* drop, void* stream);

/* ------------------------------------------------------------------------------------
 * Box decode of the box post-processor       mb/modeling/roi_heads/box_head/inference.py:40-88,
 *   mb/modeling/box_coder.py:49-95, mb/structures/bounding_box.py:214-225
 * rel_codes [num_rows, 4 * boxes_per_row] (row stride codes_row_stride, in floats), boxes [num_rows, 4] (row stride
 * boxes_row_stride) -> decoded [num_rows, 4 * boxes_per_row] dense: BoxCoder.decode with the given weights and
 * bbox_xform_clip, expression by expression as the reference writes it.  num_images > 0 also clips every row to its image
 * (clip_to_image): rows_per_image [num_images] int32 and image_wh [num_images, 2] float (width, height) are HOST arrays
 * (at most OVIS_BOX_DECODE_MAX_IMAGES images: they travel as kernel arguments), rows are image-major and
 * sum(rows_per_image) == num_rows.  One launch.
 * ---------------------------------------------------------------------------------- */
#define OVIS_BOX_DECODE_MAX_IMAGES 16
int ovis_box_decode_f32(const float* rel_codes, long codes_row_stride, const float* boxes, long boxes_row_stride,
                        long num_rows, int boxes_per_row, float weight_x, float weight_y, float weight_w,
                        float weight_h, float xform_clip, int num_images, const int32_t* rows_per_image,
                        const float* image_wh, float* decoded, void* stream);

/* ------------------------------------------------------------------------------------
 * Merge of the detections of test-time-augmentation views   mb/engine/bbox_aug.py:53-60 (flip back, resize to the first
 *   view's size, concatenate), mb/structures/bounding_box.py:91-166, mb/modeling/roi_heads/box_head/inference.py:137-143
 *   (`scores > thresh` per class)                                                                 csrc/view_merge.hip
 * boxes [num_rows, num_classes, 4] / scores [num_rows, num_classes] f32: every view's class-specific detections in the
 * view's own frame.  A SEGMENT is the contiguous rows of one (image, view); the records are HOST arrays, image-major then
 * view order: segments [num_segments, 5] int32 = (row_start, row_count >= 0, image, view_width, flip), ratios
 * [num_segments, 2] f32 = (ratio_w, ratio_h).  At most OVIS_VIEW_MERGE_MAX_SEGMENTS per call (they travel as kernel
 * arguments; more: OVIS_ERANGE); a longer list is several calls over whole images, each with its own part of `counts`.
 * Images of one call are consecutive and each owns at least one segment; rows outside [0, num_rows): OVIS_EINVAL before any
 * launch.  A box becomes ((W - x2) - 1, y1, (W - x1) - 1, y2) when flip, then (x * ratio_w, y * ratio_h), as two float
 * operations each in that order; class c >= 1 of a row is a candidate iff scores[row, c] > score_thresh (NaN: no).
 * The candidate list is ordered image, class, segment, row.  Three enqueue-only steps, one launch each:
 *   count    counts [num_counts] int32, num_counts = num_classes * sum over the call's segments of
 *            max(1, ceil(row_count / OVIS_VIEW_MERGE_TILE_ROWS)); laid out [image][class][tile of the image]
 *   scan     exclusive scan of ALL calls' counts in place (one workgroup); *total = K, the number of candidates
 *   scatter  starts = the scanned counts of this call; cand_boxes [K, 4] (16-byte aligned), cand_scores [K], cand_group [K]
 *            int32 = image * num_classes + class, offsets [num_images * num_classes (+ 1 for K, written by scan)] int32 =
 *            the start of every (image, class) run of the call's images.  Nothing is written at or beyond num_candidates.
 * The placement is count -> scan -> rank by wave64 ballot: deterministic, no atomics.  num_rows * num_classes < 2^31.
 * ---------------------------------------------------------------------------------- */
#define OVIS_VIEW_MERGE_MAX_SEGMENTS 64
#define OVIS_VIEW_MERGE_TILE_ROWS 64
int ovis_view_merge_count_f32(const float* scores, long num_rows, int num_classes, int num_images, const int32_t* segments,
                              const float* ratios, int num_segments, float score_thresh, int32_t* counts, long num_counts,
                              void* stream);
int ovis_view_merge_scan_i32(int32_t* counts, long num_counts, int32_t* total, void* stream);
int ovis_view_merge_scatter_f32(const float* boxes, const float* scores, long num_rows, int num_classes, int num_images,
                                const int32_t* segments, const float* ratios, int num_segments, float score_thresh,
                                const int32_t* starts, long num_counts, long num_candidates, float* cand_boxes,
                                float* cand_scores, int32_t* cand_group, int32_t* offsets, void* stream);

/* ------------------------------------------------------------------------------------
 * Box voting over the merged candidate list, and the mean of the views' mask maps        csrc/box_vote.hip
 *   Neither is in the reference (mb/engine/bbox_aug.py:53-69 hands out the NMS survivors, boxes only); the voting rule is
 *   Detectron's box_voting with scoring method ID.
 * vote: cand_boxes [K, 4] (16-byte aligned), cand_scores [K], cand_group [K] int32 and offsets [num_groups + 1] int32 are the
 * outputs of the view merge above; kept [num_kept] int64 are candidate indices (the detections the NMS kept).  voted
 * [num_kept, 4] (16-byte aligned) row j = sum_k s_k * box_k / sum_k s_k over the candidates k of kept[j]'s own run
 * offsets[g] .. offsets[g + 1], g = cand_group[kept[j]], with IoU(box_kept[j], box_k) >= vote_thresh -- the IoU of ovis_nms_f32
 * operand for operand, so a pair is on the same side of a threshold for the NMS and for the vote.  One wavefront per
 * detection, five float32 partial sums per lane (lane l takes candidates lo + l, lo + l + 64, ...), a fixed xor butterfly:
 * no atomics, the same bits on every call.  Every load is bounded by offsets and K: a kept index outside [0, K), a group
 * outside [0, num_groups) or a kept index outside its group's run stores 1 to *status (device int32, zeroed by the caller)
 * and a zero row, and no address is formed from it.  num_kept == 0: nothing is launched.
 * average: maps [num_views, num_maps, resolution, resolution] f32 -> out [num_maps, resolution, resolution] =
 * (((m_0 + m_1) + m_2) + ...) / float(num_views), view v's columns reversed when bit v of flip_bits is set; a division, so
 * one unflipped view returns its input bit for bit.  num_views <= 64 (more: OVIS_ERANGE).  One launch.
 * ---------------------------------------------------------------------------------- */
int ovis_vote_boxes_f32(const float* cand_boxes, const float* cand_scores, const int32_t* offsets, const int32_t* cand_group,
                        long num_candidates, int num_groups, const int64_t* kept, long num_kept, float vote_thresh,
                        float* voted, int32_t* status, void* stream);
int ovis_average_view_masks_f32(const float* maps, int num_views, long num_maps, int resolution, uint64_t flip_bits,
                                float* out, void* stream);

/* ------------------------------------------------------------------------------------
 * Soft-NMS over the candidate list (linear, Gaussian, hard)                             csrc/soft_nms.hip
 *   Not in the reference (mb/modeling/roi_heads/box_head/inference.py:121-163 suppresses greedily); the rule is Bodla et al.,
 *   "Soft-NMS -- Improving Object Detection With One Line of Code" (ICCV 2017) as Detectron's TEST.SOFT_NMS applies it.
 *   Detectron's cython soft_nms is not a dependency, so the rule is restated here in full.
 * cand_boxes [K, 4] (16-byte aligned, xyxy), cand_scores [K] and offsets [num_groups + 1] int32 are the outputs of the view
 * merge above, exactly as ovis_vote_boxes_f32 takes them: run g = the candidates offsets[g] .. offsets[g + 1] of one (image,
 * class), runs back to back, offsets[0] == 0 and offsets[num_groups] == K.  Every run is processed on its own:
 *   1. working scores w_k = s_k; every candidate is alive.
 *   2. while a candidate is alive: SELECT the alive m with the largest w; ties go to the LOWER candidate index.  m's final
 *      score is w_m, and m leaves the alive set.
 *   3. for every k still alive: ov = IoU(b_m, b_k), the float32 IoU of ovis_nms_f32 operand for operand (+1 area convention,
 *      csrc/nms.hip::iou_xyxy, the function ovis_vote_boxes_f32 uses), so a pair is on the same side of a threshold for the
 *      NMS, the vote and Soft-NMS.
 *   4. weight:  OVIS_SOFT_NMS_LINEAR    ov > nms_thresh ? 1 - ov : 1
 *               OVIS_SOFT_NMS_HARD      ov > nms_thresh ? 0 : 1
 *               OVIS_SOFT_NMS_GAUSSIAN  (float) exp(-(double) q), q = (ov * ov) / sigma: product and division in float32, the
 *               exponential in float64, rounded ONCE to float32.  (Two correct float64 exponentials agree after that rounding
 *               unless the exact value lies within a float64 ulp of a float32 midpoint; float32 expf implementations differ
 *               by an ulp routinely, and such a difference grows multiplicatively round after round.)
 *   5. w_k = w_k * weight, one float32 multiplication.  If w_k < min_score (strictly), k is DISCARDED and leaves the alive set.
 *   6. soft_scores[k] = the final score of a selected candidate, 0 for a discarded one.
 * A selected candidate always has a positive score: a working score that is not > 0 -- a product that underflows to exactly 0
 * under min_score == 0, a NaN (inf * 0), or an input score that is not > 0 to begin with -- counts as discarded.
 * sigma > 0 and min_score >= 0 (otherwise OVIS_EINVAL); method other than the three: OVIS_EINVAL.  OVIS_SOFT_NMS_HARD with
 * min_score == 0 is the greedy NMS of ovis_nms_f32 in `>` mode: soft_scores[k] = s_k for its survivors, 0 elsewhere.
 * Detectron's defaults are method linear, sigma 0.5, nms_thresh = the NMS threshold and min_score 0.0001; the callers here
 * pass MODEL.ROI_HEADS.SCORE_THRESH as min_score instead (README).
 * One launch, no workspace, no atomics.  Lane l of the T lanes that share a run owns candidates l, l + T, ... of it: a round
 * is one pass of every lane over its own candidates (decay, and the lane's next maximum on the way) and one reduction of the
 * lanes' (score, index) pairs -- a fixed xor butterfly in a wavefront, whose compare is "larger score, then lower index" and
 * therefore independent of the lane order, then one LDS slot per wavefront, double-buffered: one barrier per round.  Three
 * forms of the SAME loop, the same bits from each:
 *   run length <= OVIS_SOFT_NMS_WAVE_CANDIDATES          one wavefront per run, four runs per workgroup, no barrier; boxes and
 *                                                        working scores in LDS
 *   ... <= OVIS_SOFT_NMS_LDS_CANDIDATES                  one 256-lane workgroup per run, boxes and working scores in LDS
 *   longer                                               the workgroup form over global memory: boxes from cand_boxes, the
 *                                                        working scores in soft_scores (negated while alive)
 * OVIS_SOFT_NMS_LDS_CANDIDATES: 20 bytes per candidate (box + working score) and the reduction slots within 40 KiB, a quarter
 * of gfx950's 160 KiB of LDS per CU: four workgroups (16 wavefronts) stay resident per CU.
 * Every load is bounded by offsets and K.  offsets[0] != 0, a negative or decreasing entry, an entry above K or
 * offsets[num_groups] != K stores 1 to *status (device int32, zeroed by the caller): the runs in front of the first such
 * entry are processed as usual, every candidate from there on gets 0, and no address is formed from a bad value.
 * num_candidates == 0 or num_groups == 0: nothing is launched.
 * ---------------------------------------------------------------------------------- */
#define OVIS_SOFT_NMS_LINEAR 0
#define OVIS_SOFT_NMS_GAUSSIAN 1
#define OVIS_SOFT_NMS_HARD 2
#define OVIS_SOFT_NMS_WAVE_CANDIDATES 256
#define OVIS_SOFT_NMS_LDS_CANDIDATES 2032
int ovis_soft_nms_f32(const float* cand_boxes, const float* cand_scores, const int32_t* offsets, long num_candidates,
                      int num_groups, int method, float nms_thresh, float sigma, float min_score, float* soft_scores,
                      int32_t* status, void* stream);

/* Pooler.convert_to_roi_format (mb/modeling/poolers.py:73-86): boxes[i] (HOST array of device pointers) holds image i's
 * [boxes_per_image[i], 4] boxes (boxes_per_image: HOST array); rois [sum, 5] receives (id_i, x1, y1, x2, y2) rows in list
 * order, id_i = image_ids[i] (HOST array) or i when image_ids is NULL.  One launch per OVIS_BOX_DECODE_MAX_IMAGES images. */
int ovis_rois_from_boxes_f32(const float* const* boxes, const int32_t* boxes_per_image, const int32_t* image_ids,
                             int num_images, float* rois, void* stream);

/* ------------------------------------------------------------------------------------
 * Box-regression loss of the box head, forward + backward fused
 *   mb/modeling/roi_heads/box_head/loss.py:147-170, mb/layers/smooth_l1_loss.py:6-16
 * loss[0] = sum over the positives p = positives[0..num_positives) and c < 4 of
 *   smooth_l1(box_regression[p, col0(p) + c] - regression_targets[p, c]; beta) / denominator,
 * col0(p) = 4 * labels[p] (labels != NULL: class-specific regression) or column0 (class-agnostic: 4).
 * grad_regression (may be NULL) [num_rows, num_columns] dense is fully written (zero outside the picked entries).
 * Single workgroup, fixed summation order: deterministic.
 * ---------------------------------------------------------------------------------- */
int ovis_smooth_l1_picked_fwd_bwd_f32(const float* box_regression, long regression_row_stride, int num_rows,
                                      int num_columns, const float* regression_targets, long targets_row_stride,
                                      const int64_t* positives, const int64_t* labels, int num_positives, int column0,
                                      float beta, float denominator, float* loss, float* grad_regression, void* stream);

/* ------------------------------------------------------------------------------------
 * ROIPool                                    mb/csrc/ROIPool.h:11-48
 *   kernels: mb/csrc/cuda/ROIPool_cuda.cu:17-77 (fwd), :80-108 (bwd)
 * input [batch, channels, height, width] f32, rois [num_rois, 5] (batch index, x1, y1, x2, y2);
 * output / argmax [num_rois, channels, pooled_h, pooled_w] (f32 max per bin / int32 index into the
 * H*W plane, -1 for an empty bin whose value is 0).  Backward fully writes grad_input
 * [batch, channels, height, width] (zero fill + scatter-add to the argmax positions).
 * ---------------------------------------------------------------------------------- */
int ovis_roi_pool_forward_f32(const float* input, const float* rois, float* output, int32_t* argmax,
                              int num_rois, int batch, int channels, int height, int width,
                              int pooled_h, int pooled_w, float spatial_scale, void* stream);
int ovis_roi_pool_backward_f32(const float* grad_output, const int32_t* argmax, const float* rois,
                               float* grad_input, int num_rois, int batch, int channels, int height,
                               int width, int pooled_h, int pooled_w, void* stream);

/* ------------------------------------------------------------------------------------
 * Deformable position-sensitive RoI pooling  mb/csrc/deform_pool.h:11-70
 *   kernels: mb/csrc/cuda/deform_pool_kernel_cuda.cu:31-139 (fwd), :141-263 (bwd); host: deform_pool_cuda.cu:38-90
 * data [batch, channels, height, width] f32; rois [num_rois, 5] (batch index, x1, y1, x2, y2);
 * trans [num_rois, channels_trans, part_size, part_size] (channels_trans = 2 * classes; ignored when no_trans);
 * out / out_count [num_rois, output_dim, pooled_size, pooled_size]: the mean of the bilinear samples of every bin that
 * fall inside the map, read from plane (ctop * group_size + gh) * group_size + gw, and their number (f32, as upstream).
 * Backward ACCUMULATES into grad_data (and grad_trans unless no_trans): the caller zero-fills them, as the reference's
 * autograd function does (layers/dcn/deform_pool_func.py:68-70).
 * ---------------------------------------------------------------------------------- */
int ovis_deform_psroi_pool_forward_f32(const float* data, const float* rois, const float* trans, float* out,
                                       float* out_count, int num_rois, int batch, int channels, int height, int width,
                                       int channels_trans, int no_trans, float spatial_scale, int output_dim,
                                       int group_size, int pooled_size, int part_size, int sample_per_part,
                                       float trans_std, void* stream);
int ovis_deform_psroi_pool_backward_f32(const float* grad_out, const float* out_count, const float* data,
                                        const float* rois, const float* trans, float* grad_data, float* grad_trans,
                                        int num_rois, int batch, int channels, int height, int width,
                                        int channels_trans, int no_trans, float spatial_scale, int output_dim,
                                        int group_size, int pooled_size, int part_size, int sample_per_part,
                                        float trans_std, void* stream);

/* ------------------------------------------------------------------------------------
 * Sigmoid focal loss                         mb/csrc/SigmoidFocalLoss.h:10-41
 *   kernels: mb/csrc/cuda/SigmoidFocalLoss_cuda.cu:21-58 (fwd), :62-101 (bwd)
 * logits [num, num_classes] f32; targets [num] int32 (-1 ignore, 0 background,
 * j+1 = positive for column j); losses / d_logits [num, num_classes] f32.
 * ---------------------------------------------------------------------------------- */
int ovis_sigmoid_focal_loss_forward_f32(const float* logits, const int32_t* targets,
                                        float* losses, int num, int num_classes,
                                        float gamma, float alpha, void* stream);
int ovis_sigmoid_focal_loss_backward_f32(const float* logits, const int32_t* targets,
                                         const float* d_losses, float* d_logits, int num,
                                         int num_classes, float gamma, float alpha,
                                         void* stream);

/* ------------------------------------------------------------------------------------
 * bf16 hi/lo operand split for fp32-accurate GEMMs on the bf16 matrix pipe ("next" row f-1:
 * the res5 1x1 convolutions, mb/modeling/backbone/resnet.py:239-344, as NHWC GEMMs).
 * src [rows, cols] f32 (row stride in elements) -> dst [rows, 3*cols] bf16 with row layout
 * [hi | hi | lo] (mode 0, left operand) or [hi | lo | hi] (mode 1, right operand), hi =
 * bf16(x), lo = bf16(x - hi): a plain bf16 GEMM over the 3*cols columns of a mode-0 and a
 * mode-1 operand is the three-term product hi.hi + hi.lo + lo.hi (~4e-6 relative error).
 * cols and the row stride must be multiples of 4, src 16-byte and dst 8-byte aligned
 * (else OVIS_ERANGE: use the fp32 GEMM).
 * ---------------------------------------------------------------------------------- */
int ovis_split_bf16x3_f32(const float* src, long src_row_stride, void* dst_bf16, long rows,
                          int cols, int mode, void* stream);

/* Split + im2col of an NHWC tensor for odd-sized stride-1 "same" convolutions as bf16 GEMMs:
 * src [num, height, width, channels] f32 -> dst [num*height*width, 3*T*channels] bf16 with
 * T = kh*kw taps and row layout [hi(tap 0..T-1) | hi(tap 0..T-1) | lo(tap 0..T-1)]; tap
 * (ky, kx) reads pixel (y + ky - kh/2, x + kx - kw/2), zeros outside the map; flip != 0
 * takes the taps in reverse order (180-degree rotated kernel of the data gradient).
 * A bf16 GEMM of dst against the mode-1 split of the [Cout, T*channels] weight matrix is the
 * convolution (res5 conv2, mb/modeling/backbone/resnet.py:288-300).  channels % 4 == 0. */
int ovis_im2col_split_bf16x3_f32(const float* src, void* dst_bf16, long num, int height,
                                 int width, int channels, int kh, int kw, int flip, void* stream);

/* Fused GEMM epilogue of the NHWC res5 head: y[rows, cols] = act(y + bias[col] (+ residual)) in
 * place, act = ReLU when `relu` != 0 (Bottleneck.forward, mb/modeling/backbone/resnet.py:323-344:
 * FrozenBN shift, shortcut add and ReLU in one pass).  bias / residual may be NULL; cols % 4 == 0
 * and 16-byte aligned pointers (else OVIS_ERANGE). */
int ovis_bias_act_f32(float* y, const float* bias, const float* residual, long rows, int cols,
                      int relu, void* stream);

/* ------------------------------------------------------------------------------------
 * Pair-layout split GEMM / implicit-GEMM convolution (csrc/split_gemm.hip): the res5 head and the
 * frozen trunk (Bottleneck.forward, mb/modeling/backbone/resnet.py:323-344; ResNetHead :155-204)
 * as fp32-accurate products on the bf16 matrix cores, with the operand split shared by the three
 * hi/lo products inside the kernel.
 *
 * PAIR LAYOUT of a row of K fp32 values (K % 32 == 0): K/32 blocks of 128 bytes, each
 * [hi(32 x bf16) | lo(32 x bf16)], hi = bf16(x), lo = bf16(x - hi); 4*K bytes per row.
 * ---------------------------------------------------------------------------------- */
/* src [rows, cols] f32 (row stride in elements) -> dst pair rows (4*cols bytes each, dense).
 * cols % 32 == 0, stride % 4 == 0, 16-byte aligned pointers (else OVIS_ERANGE). */
int ovis_split_pair_f32(const float* src, long src_row_stride, void* dst_pair, long rows,
                        int cols, void* stream);

/* Backward ReLU gate fused with the operand split: g = dy * (y > 0) -> dst_pair (pair rows, dense) and, when
 * g_f32 != NULL, also as dense fp32.  dy [rows, cols] f32 (row stride in elements); gate = the saved forward
 * output y, dense: its pair form (gate_is_pair != 0; only the hi halves are read) or fp32, or NULL (no gate:
 * a plain split).  threshold_backward of mb/modeling/backbone/resnet.py:323-344's relu_ calls.  cols % 32 == 0.
 * The two gate forms agree for every positive NORMAL y; for 0 < y <= 2^-134 the pair form gates to zero, because hi
 * rounds to 0, and the fp32 form passes.
 * g_pooled != NULL: [rows / pool_rows, cols] f32, the gradient of the mean over every pool_rows consecutive rows
 * (the 7x7 average pooling of FastRCNNPredictor.forward, roi_box_predictors.py:62-66, behind the res5 head) is
 * added on the fly, g = (dy + g_pooled[row / pool_rows] / pool_rows) * (y > 0); dy may then be NULL.
 * g_selected != NULL: the gradient of a ROW-GROUP GATHER is added on the fly as well: the rows come in groups of
 * pool_rows (the 7x7 positions of one RoI); group_slot [rows / pool_rows] int32 holds, for a group that a consumer gathered (the mask
 * head reads the res5 features of the positive RoIs only: mb/modeling/roi_heads/mask_head/mask_head.py:13-41,62-66),
 * its index in g_selected [num_selected * pool_rows, cols] f32 (dense), -1 otherwise:
 * g = (dy + g_pooled[group] / pool_rows + g_selected[group_slot[group] * pool_rows + row in group]) * (y > 0).
 * Replaces the zero-filled [rows, cols] tensor an index backward would build and this kernel would read back.
 * dy, g_pooled may be NULL; g_selected and group_slot are given together. */
int ovis_gate_split_pair_rows_f32(const float* dy, long dy_row_stride, const void* gate, int gate_is_pair,
                                  void* dst_pair, float* g_f32, long rows, int cols, const float* g_pooled,
                                  int pool_rows, const float* g_selected, const int32_t* group_slot, void* stream);

/* Weight preparation of a (trainable) convolution in one launch: weight [out_channels, in_channels, taps] f32 times the
 * folded FrozenBN scale [out_channels] (may be NULL; mb/layers/batch_norm.py:19-31) -> fwd_pair [out_channels, taps*in]
 * pair rows, k = tap*in + c (the forward / weight-gradient layout) and, when bwd_pair != NULL, [in_channels, taps*out]
 * pair rows, k' = tap*out + n (the data-gradient operand).  in_channels % 32 == 0 (out_channels too for bwd_pair). */
int ovis_weight_prep_pair_f32(const float* weight, const float* scale, void* fwd_pair, void* bwd_pair,
                              int out_channels, int in_channels, int taps, void* stream);

/* dweight [out, in, taps] = scale[out] * sum over the slabs of ovis_split_gemm_pair_tn ([slices, out, taps*in]). */
int ovis_slab_reduce_f32(const float* slabs, const float* scale, float* dweight, int slices, int out_channels,
                         int in_channels, int taps, void* stream);

/* Pair-layout im2col (the M-contracting weight gradient of a 3x3 needs the rows materialised):
 * src NHWC [num, height, width, channels] pair rows -> dst [num*height*width, kh*kw*channels]
 * pair rows, tap-major, zero rows for taps outside the map.  channels % 32 == 0. */
int ovis_im2col_pair(const void* src_pair, void* dst_pair, long num, int height, int width,
                     int channels, int kh, int kw, void* stream);

/* ovis_split_gemm_pair for a data gradient whose result passes a ReLU gate: C = (A B^T) * (y > 0) with y the forward
 * activation in pair layout (gate_pair, rows gate_row_bytes apart; only the hi halves are read), written as fp32 (c)
 * and / or in pair layout (c_pair) -- the gate and the operand split of the NEXT backward GEMM in this epilogue.
 * n % 32 == 0.
 * workspace: split-K scratch (size: ovis_split_gemm_pair_workspace_bytes(m, n, channels, 0, taps_h, taps_w, width);
 * NULL / too small = the un-split grid): grids that leave most CUs idle while every workgroup walks a long K (the data
 * gradients of a trainable trunk on 50 x 84 maps) are cut into K slices as in ovis_split_gemm_pair; the slab reduction
 * applies the gate and writes c / c_pair.  Same results as the un-split grid up to the fp32 summation order of the slices
 * (fixed: reproducible). */
int ovis_split_gemm_pair_gated_ws(const void* a_pair, long a_row_bytes, const void* b_pair, long b_row_bytes,
                                  float* c, long ldc, void* c_pair, long c_pair_row_bytes, const void* gate_pair,
                                  long gate_row_bytes, long m, int n, int channels, int taps_h, int taps_w,
                                  int height, int width, int flip, void* workspace, size_t workspace_bytes,
                                  int config, void* stream);

/* The input gradient of an identity bottleneck (mb/modeling/backbone/resnet.py:290-342: out = relu(conv3(..) + x)), handed
 * to the block below ready for use: C = (A B^T + r) * (x > 0) -- r the gradient arriving through the shortcut, given in
 * pair layout (residual_pair: hi + lo), x the block input in pair layout (gate_pair: the block below's ReLU output, only
 * the hi halves are read) -- written in pair layout (c_pair) and / or fp32 (c).  The block below then needs neither a
 * gate + split pass nor an fp32 gradient tensor.  Plain products only (1x1); n % 32 == 0, n >= 128 (else OVIS_ERANGE). */
int ovis_split_gemm_pair_rp_gated(const void* a_pair, long a_row_bytes, const void* b_pair, long b_row_bytes, float* c,
                                  long ldc, void* c_pair, long c_pair_row_bytes, const void* residual_pair,
                                  long residual_pair_row_bytes, const void* gate_pair, long gate_row_bytes, long m, int n,
                                  int channels, int config, void* stream);

/* im2col of a strided convolution on an NCHW f32 image [num, channels, height, width] into pair rows
 * [num*ho*wo, k_padded]: k = (ky*kw + kx)*channels + c, columns >= kh*kw*channels are zero (k_padded % 32 == 0).
 * The 7x7 stride-2 stem (mb/modeling/backbone/resnet.py:347-366) then is one ovis_split_gemm_pair. */
int ovis_im2col_nchw_pair_f32(const float* src, void* dst_pair, int num, int channels, int height, int width,
                              int kh, int kw, int stride, int pad, int k_padded, void* stream);

/* C[m, n] = act( sum_{tap, c} A[row(m, tap), c] * B[n, tap*channels + c] (+ sum_c A2[m, c] * B[n, channels + c])
 *                + bias[n] + residual[m, n] )
 *   a_pair : pair rows of `channels` values, a_row_bytes apart.  taps_h = taps_w = 1: a plain
 *            [m, channels] matrix.  Otherwise an NHWC tensor [m / (height*width), height, width,
 *            channels]; tap (ty, tx) of row (r, y, x) reads pixel (y + ty - taps_h/2, x + tx -
 *            taps_w/2) (negated offsets when flip != 0: the data-gradient convolution), zeros
 *            outside the map -- stride-1 "same" convolution with no im2col matrix.  Maps whose largest
 *            tap shift (taps_h/2)*width + taps_w/2 is <= 8 rows (the 7x7 maps of the res5 head) are
 *            staged once per channel block with a halo and read by all taps from LDS.
 *   a2_pair: optional second operand (taps 1x1 only; NULL / channels2 = 0 otherwise): [m, channels2] pair
 *            rows whose products follow a_pair's along K, b_pair then holds channels + channels2 values
 *            per row -- conv3 + projection shortcut of a bottleneck (mb/modeling/backbone/resnet.py:
 *            323-344) as ONE product, the shortcut tensor is never written.
 *   b_pair : n pair rows of taps*channels (+ channels2) values (weights [n, tap, c]), b_row_bytes apart.
 *   c      : fp32 result, row stride ldc elements, or NULL;  c_pair: the result in pair layout
 *            (rows c_pair_row_bytes apart; needs n % 32 == 0), or NULL -- the operand split of the
 *            NEXT layer fused into this epilogue.  bias [n] / residual [m, n] (stride ldr) may be NULL.
 *   workspace : ovis_split_gemm_pair_workspace_bytes(...) bytes (16-byte aligned) or NULL.  Problems with few
 *            output tiles and a long K (the pseudo-box passes: m = a few hundred rows) are cut along K into
 *            slices whose partial tiles go to fp32 slabs in the workspace; a second launch sums them and
 *            applies the epilogue (deterministic).  Without a workspace the un-split grid runs.
 *   config : 0 = choose.  Otherwise a bit set for tests and A/B measurements: 1 = one LDS stage, 2 = two
 *            stages, 4 = never use the halo form, 8 = no K slices.
 * channels % 32 == 0, channels2 % 32 == 0, n % 4 == 0, 16-byte aligned pointers and strides (else OVIS_ERANGE).
 * More than one tap: m is a multiple of height * width (whole maps; the rows of a partial last map would read their taps
 * behind a_pair), else OVIS_EINVAL before any launch -- also through ovis_split_gemm_pair_gated_ws. */
size_t ovis_split_gemm_pair_workspace_bytes(long m, int n, int channels, int channels2, int taps_h, int taps_w,
                                            int width);
/* The same query for a launch with a non-zero `config` (bit 16 = co-scheduled launch: slices chosen for least total work;
 * bits 8..15 = forced slice count): the plan, and with it the slabs' size, follows config. */
size_t ovis_split_gemm_pair_workspace_bytes_ex(long m, int n, int channels, int channels2, int taps_h, int taps_w,
                                               int width, int config);
int ovis_split_gemm_pair(const void* a_pair, long a_row_bytes, const void* a2_pair, long a2_row_bytes,
                         const void* b_pair, long b_row_bytes, float* c, long ldc, void* c_pair,
                         long c_pair_row_bytes, const float* bias, const float* residual, long ldr, long m,
                         int n, int channels, int channels2, int taps_h, int taps_w, int height, int width,
                         int flip, int relu, void* workspace, size_t workspace_bytes, int config, void* stream);
/* The plain (1x1) form with the shortcut operand in PAIR layout: residual_pair [m, n] pair rows (n % 32 == 0), added as
 * hi + lo (exact in fp32; 2^-17 relative to the value the pair was split from).  A bottleneck
 * (mb/modeling/backbone/resnet.py:323-344) holds its input as the pair operand of conv1 anyway: with this form the
 * identity shortcut needs no fp32 copy of the block input, so the producing block writes its result in pair layout only. */
int ovis_split_gemm_pair_rp(const void* a_pair, long a_row_bytes, const void* b_pair, long b_row_bytes, float* c, long ldc,
                            void* c_pair, long c_pair_row_bytes, const float* bias, const void* residual_pair,
                            long residual_pair_row_bytes, long m, int n, int channels, int relu, void* workspace,
                            size_t workspace_bytes, int config, void* stream);

/* Weight gradient on pair operands: c_slabs[s][n][tap*channels + c] = sum over the rows m of slice s of
 * G[m, n] * X[row(m, tap), c]  (G = gated output gradient [m, n], X = the layer input [m, channels], both pair
 * rows; taps as in ovis_split_gemm_pair, X read shifted with zeros outside the map).  The rows are cut into
 * `slices` (ovis_split_gemm_tn_slices gives a count that fills the chip); the caller sums the slabs.
 * n % 128 == 0, channels % 128 == 0 (else OVIS_ERANGE); any map size, but whole maps: with more than one tap m is a
 * multiple of height * width (the rows of a partial last map would read X behind the operand), else OVIS_EINVAL before
 * any launch.  A slice count above the number of 32-row steps is served: the slabs of the empty slices are zero-filled.
 * On maps of at most 64 pixels (m a multiple of height * width, at most 5 x 5 taps) a tap contracts over its in-map rows
 * only, every tap is cut into `slices` slices of its own rows and the taps with the most rows are dispatched first;
 * the slab layout is the same.  ovis_split_gemm_tn_map_slices scores that work (and equals ovis_split_gemm_tn_slices
 * for every other shape). */
int ovis_split_gemm_tn_slices(long m, int n, int channels, int taps);
int ovis_split_gemm_tn_map_slices(long m, int n, int channels, int taps_h, int taps_w, int height, int width);
int ovis_split_gemm_pair_tn(const void* g_pair, long g_row_bytes, const void* x_pair, long x_row_bytes,
                            float* c_slabs, int slices, long m, int n, int channels, int taps_h,
                            int taps_w, int height, int width, void* stream);

/* ------------------------------------------------------------------------------------
 * Training-target construction on the device (csrc/targets.hip), one launch per image instead of ~100 tensor ops.
 *
 * ovis_match_encode_f32: boxlist_iou (mb/structures/boxlist_ops.py:53-89) of gt_boxes [num_gt,4] x proposals
 * [num_proposals,4] -> Matcher without low-quality matches (mb/modeling/matcher.py:42-81) -> matched_idx
 * [num_proposals] (argmax gt, 0 when below/between the thresholds, i.e. matched.clamp(min=0)), labels (gt label;
 * 0 below low_threshold; between the thresholds -1 [between_keeps_label == 0, box head: box_head/loss.py:60-70] or
 * the label of gt 0 [!= 0, mask head: mask_head/loss.py:60-77]) and, when regression_targets != NULL, BoxCoder.encode
 * (mb/modeling/box_coder.py:22-52) of the matched gt box with weights (wx, wy, ww, wh).
 *
 * ovis_project_masks_f32: project_masks_on_boxes (mb/modeling/roi_heads/mask_head/loss.py:11-42) for binary masks
 * [G, height, width] (1 byte per pixel; bool or uint8): crop to the rounded box, bilinear resize to resolution^2
 * (align_corners = False), cast back to the mask dtype -> out [num, resolution, resolution] f32.
 * ---------------------------------------------------------------------------------- */
int ovis_match_encode_f32(const float* gt_boxes, const int64_t* gt_labels, const float* proposals, int num_gt,
                          int num_proposals, float high_threshold, float low_threshold, int between_keeps_label,
                          float wx, float wy, float ww, float wh, int64_t* matched_idx, int64_t* labels,
                          float* regression_targets, void* stream);
/* ovis_rpn_match_encode_f32: the RPN's target building (mb/modeling/rpn/loss.py:21-89) for one image: boxlist_iou of
 * gt_boxes [num_gt, 4] x anchors [num_anchors, 4] -> Matcher WITH low-quality matches (mb/modeling/matcher.py:42-112: an
 * anchor whose IoU equals a ground truth's best IoU keeps its argmax; pass 1 takes the per-ground-truth maxima into
 * best_per_gt_scratch [num_gt] uint32, pass 2 compares bit patterns) -> labels [num_anchors] int64: 1 matched, 0 below the
 * low threshold, -1 ignored (between the thresholds, or visibility[a] == 0: anchors straddling the image border), in the
 * reference's order of the three rules; regression_targets [num_anchors, 4] = BoxCoder.encode of the matched ground truth
 * (index clamped at 0) with weights (wx, wy, ww, wh).  allow_low_quality_matches == 0: the plain Matcher. */
int ovis_rpn_match_encode_f32(const float* gt_boxes, const float* anchors, const uint8_t* visibility, int num_gt,
                              int num_anchors, float high_threshold, float low_threshold, int allow_low_quality_matches,
                              float wx, float wy, float ww, float wh, uint32_t* best_per_gt_scratch, int64_t* labels,
                              float* regression_targets, void* stream);
int ovis_project_masks_f32(const uint8_t* masks, const int64_t* gt_index, const float* boxes, int num, int height,
                           int width, int resolution, int masks_are_bool, float* out, void* stream);
/* ovis_sample_fg_bg: BalancedPositiveNegativeSampler of one image (mb/modeling/balanced_positive_negative_sampler.py:
 * 19-68) in one launch.  labels [num] int64 (>= 1 positive, 0 negative, < 0 ignored).  num_pos = min(#positives,
 * max_positives), num_neg = min(#negatives, batch_size - num_pos); a uniformly random subset of each size (keys =
 * splitmix64(seed, index): the reference draws torch.randperm()[:k], whose stream is version dependent) -> selected
 * [batch_size] int64: the chosen indices ASCENDING (the order of the reference's nonzero(pos_mask | neg_mask)), zeros
 * behind them; positive_slots [batch_size]: positions of the positives inside `selected`; counts[0] = number selected,
 * counts[1] = positives among them.  No host round trip.
 *
 * ovis_project_pasted_masks_f32: ovis_project_masks_f32 for ground truths whose binary image mask is DEFINED by a
 * prob_resolution^2 probability map and a box -- Masker.forward_single_image (mb/modeling/roi_heads/mask_head/
 * inference.py:100-160, padding 1: pad, expand the box by (M+2)/M, truncate to integers, bilinear resize, > threshold,
 * paste clipped to the image) -- as the pseudo labels' masks are (st_generalized_rcnn.py:266-271).  Every mask pixel
 * the crop + resize reads is evaluated from the map on the fly: same targets as pasting first, no H x W canvas.
 * mask_probs [G, prob_resolution, prob_resolution] f32, gt_boxes [G, 4], gt_index [num], boxes [num, 4]. */
int ovis_sample_fg_bg(const int64_t* labels, int num, int batch_size, int max_positives, uint64_t seed,
                      int64_t* selected, int64_t* positive_slots, int32_t* counts, void* stream);
int ovis_project_pasted_masks_f32(const float* mask_probs, const float* gt_boxes, const int64_t* gt_index,
                                  const float* boxes, int num, int image_height, int image_width, int prob_resolution,
                                  int resolution, float threshold, float* out, void* stream);
/* ovis_branch_roi_union: the union of the RoIs two branches sampled (ovis_sample_fg_bg) from proposal lists of the same
 * images -- the student's pseudo-label and ground-truth branches (st_generalized_rcnn.py:284-408), whose lists come out of
 * one decode + NMS pass, so that the pooler and the res5 head run once per distinct RoI.  One launch for all images, no
 * host read: per image i and branch b the HOST arrays (at most OVIS_BOX_DECODE_MAX_IMAGES entries) give the DEVICE
 * pointers boxes_b[i] [num_b[i], 4] f32 (16-byte aligned), selected_b[i] / positive_slots_b[i] [batch_b] int64 and
 * counts_b[i] [2] int32 as ovis_sample_fg_bg wrote them; sampled row r of a branch is the box boxes[selected[r]].
 *   match: branch-1 row j is branch-0 row i of the SAME image when the four box words are equal as 32-bit patterns
 *          (-0.0 != 0.0, a NaN equals only its own bits), i is the lowest such row and no branch-1 row below j has
 *          those words (further equal branch-1 rows stay rows of their own): both row maps are injective.
 *   union: every branch-0 row, image-major in its order (rows [0, sum n0)), then the unmatched branch-1 rows,
 *          image-major in their order.
 *   rois [rois_rows >= num_images * (batch0 + batch1), 5]: (image_ids[i] or i, x1, y1, x2, y2) of the union rows; every
 *          row behind them is a copy of the last one (the caller may round the RoI count up).
 *   map1 [num_images * batch1] int64: the union row of every branch-1 row, image-major, dense.
 *   positive_rows [num_images * (batch0 + batch1)] int64: ascending, the union rows that are positive in either branch;
 *   slots0 [num_images * batch0] / slots1 [num_images * batch1]: each branch's positives (image-major, in the order of
 *          positive_slots) as positions in positive_rows.
 *   out_counts [num_images, 2] int32: (new rows, entries of positive_rows) the image contributed.
 *   workspace [batch0] int32.
 * Counts are clipped to the buffer lengths, proposal indices clamped into their list, slots outside the sampled rows
 * skipped: no access leaves a buffer whatever lies behind the counts.  Orders come from workgroup scans, no atomics: the
 * same words on every call. */
int ovis_branch_roi_union(const float* const* boxes0, const int32_t* num0, const int64_t* const* selected0,
                          const int64_t* const* positive_slots0, const int32_t* const* counts0,
                          const float* const* boxes1, const int32_t* num1, const int64_t* const* selected1,
                          const int64_t* const* positive_slots1, const int32_t* const* counts1, const int32_t* image_ids,
                          int num_images, int batch0, int batch1, float* rois, int rois_rows, int64_t* map1,
                          int64_t* positive_rows, int64_t* slots0, int64_t* slots1, int32_t* workspace,
                          int32_t* out_counts, void* stream);
/* ovis_paste_masks_u8: the image-size binary masks themselves -- Masker.forward_single_image / paste_mask_in_image
 * (mb/modeling/roi_heads/mask_head/inference.py:100-205, padding 1) for ALL masks of an image in one launch, with the
 * per-pixel arithmetic of ovis_project_pasted_masks_f32 (csrc/pasted_geom.h).  mask_probs [num, prob_resolution,
 * prob_resolution] f32, boxes [num, 4] xyxy (16-byte aligned), out [num, image_height, image_width] uint8 in {0, 1}
 * (the storage of a bool tensor); EVERY byte of out is written exactly once, so out needs no fill.  Enqueues only.
 * prob_resolution <= 120, num <= 65535, image_height * image_width < 2^31, else OVIS_ERANGE. */
int ovis_paste_masks_u8(const float* mask_probs, const float* boxes, int num, int prob_resolution, int image_height,
                        int image_width, float threshold, uint8_t* out, void* stream);
/* ovis_pasted_rle_*: the COCO run-length encodings of the masks ovis_paste_masks_u8 would write, without writing them --
 * prepare_for_coco_segmentation (mb/data/datasets/evaluation/coco/coco_eval.py:108-162: Masker paste, copy to the host,
 * pycocotools' encode per mask) for a chunk of images in three launches and two small host reads.  Mask p is
 * (mask_probs[p] [prob_resolution, prob_resolution] f32, boxes[p] xyxy in the frame of its image (the array 16-byte
 * aligned), image_sizes[p] = (height, width) int32), thresholded with `>`; its pixels are those of ovis_paste_masks_u8
 * (csrc/pasted_geom.h), bit for bit.  Runs: pycocotools' rleEncode -- column-major, zeros first, so a mask whose pixel
 * (0, 0) is set starts with a count of 0, an empty one is [height * width].  Text: pycocotools' rleToString.  The order
 * of every output comes from scans: no atomics, the same bytes on every call.
 *   _count:  num_runs[p] = the number of counts of mask p (>= 1), or -1 when image_sizes[p] has height < 1, width < 1 or
 *            height * width > 0x7fffffef (such a mask is skipped by _runs; the caller refuses it).
 *   _runs:   run_offsets [num + 1] int64 = the exclusive sum of num_runs (made by the caller); runs[run_offsets[p] ..
 *            run_offsets[p + 1]) = the counts of mask p, int32; never written outside that range.  num_chars[p] = the
 *            length of its compressed string (NULL: not computed).
 *   _string: char_offsets [num + 1] int64 = the exclusive sum of num_chars; out[char_offsets[p] .. char_offsets[p + 1]) =
 *            the `counts` string of mask p (ASCII, not terminated).
 * Enqueue only.  num == 0: OVIS_OK without a launch.  prob_resolution <= 120, num <= 65535, else OVIS_ERANGE. */
int ovis_pasted_rle_count(const float* mask_probs, const float* boxes, const int32_t* image_sizes, int num,
                          int prob_resolution, float threshold, int32_t* num_runs, void* stream);
int ovis_pasted_rle_runs(const float* mask_probs, const float* boxes, const int32_t* image_sizes, int num,
                         int prob_resolution, float threshold, const int64_t* run_offsets, int32_t* runs,
                         int32_t* num_chars, void* stream);
int ovis_pasted_rle_string(const int32_t* runs, const int64_t* run_offsets, const int64_t* char_offsets, int num,
                           uint8_t* out, void* stream);
/* ovis_render_instances_u8: the prediction compositor -- overlay_boxes, overlay_filled_mask and overlay_uncertainty_mask
 * (mb/engine/inference.py:519-540, :557-569, :571-589) over the Masker paste (mb/modeling/roi_heads/mask_head/
 * inference.py:124-165, padding 1; thresholded for fills, un-thresholded :150-155 for heat) in ONE launch, without building
 * a [num_layers, height, width] mask: every byte of out is written once, a pixel evaluates only the layers whose integer
 * pasted box covers it.  image, out: uint8 [height, width, 3] (HWC); out must not overlap image (OVIS_EINVAL).
 *
 * Layer i = (maps[i] [M, M] f32, boxes[i] xyxy f32 (the array 16-byte aligned), kinds[i], params[i], colors[i] [3] f32 in
 * 0..255).  The layers are applied to a pixel in INDEX order, the pixel truncated to uint8 after each (the reference
 * assigns into a uint8 array layer by layer).  v = the pasted value at the pixel (csrc/pasted_value.h: the bilinear value
 * of the zero-padded map resized to the integer pasted box; zero outside that box and outside the image):
 * A layer touches ONLY the pixels of its integer pasted box clipped to the image -- a fill with a negative params[i] does
 * not spill over the rest of the image, where v is zero.  Inside that box:
 *   kinds[i] == 0, fill:  where v > params[i]:  p <- (uint8) trunc(p * (1 - alpha) + alpha * colors[i][c]) in DOUBLE
 *                         (NumPy's `uint8 * 0.5 + 0.5 * c`; in float32 the sum can round across an integer)
 *   kinds[i] == 1, heat:  m = min(max(v * params[i], 0), 1), params[i] = float32(0.2 / score);  where m != 0:
 *                         p <- (uint8) trunc((float) p * (1 - m) + m * colors[i][c]) in FLOAT32, one rounding per operation
 *                         (NumPy's `uint8 * float32`)
 *   any other kind: the layer is skipped.  A box with a coordinate that is NaN or beyond +-1e6 has neither layer nor outline.
 * Outlines (outline_colors [num_layers, 3] uint8, NULL = none) are ALL drawn before any layer, in index order.  THE RULE,
 * ours (cv2's coverage of a thick rectangle is not reproduced): the box corners are truncated toward zero and ordered
 * (xa <= xb, ya <= yb); with thickness t an edge at integer coordinate c covers c - floor(t/2) ... c + ceil(t/2) - 1 across
 * its direction, and runs along its direction from the low end of the first corner's band to the high end of the second's
 * (filled square corners); clipped to the image.
 * num_layers == 0 copies the image.  0 <= alpha <= 1, outline_thickness >= 1 (when outlines are drawn), else OVIS_EINVAL;
 * map_resolution <= 120, height, width <= 65535, outline_thickness <= 255, else OVIS_ERANGE.  Enqueues only. */
int ovis_render_instances_u8(const uint8_t* image, int height, int width, const float* maps, const float* boxes,
                             int num_layers, int map_resolution, const int32_t* kinds, const float* params,
                             const float* colors, float alpha, const uint8_t* outline_colors, int outline_thickness,
                             uint8_t* out, void* stream);
/* ovis_gather_rows: out[i] = src[index[i]] for up to two [P, 4] f32 arrays and two [P] int64 arrays at once (a NULL source
 * is skipped) -- the sampled proposals' boxes, regression targets, labels and matched ground truths
 * (mb/modeling/roi_heads/box_head/loss.py:112-121 indexes every field of the BoxList separately).  One launch. */
int ovis_gather_rows(const int64_t* index, int num, const float* boxes_a, float* boxes_a_out, const float* boxes_b,
                     float* boxes_b_out, const int64_t* ints_a, int64_t* ints_a_out, const int64_t* ints_b,
                     int64_t* ints_b_out, void* stream);

/* ------------------------------------------------------------------------------------
 * Cross-modal head: fp32 GEMM on the matrix cores
 *   mb/modeling/roi_heads/box_head/roi_box_predictors.py:66-71 (emb_pred Linear, einsum('pe,ce->pc'),
 *   bbox_pred Linear) and their autograd transposes.
 * C[m,n] = sum_k A(m,k) * B(n,k) (+ bias[n]);  A(m,k) = A[m*a_row_stride + k*a_k_stride], B likewise,
 * C row-major with row stride c_row_stride.  Exact fp32 (v_mfma_f32_32x32x2_f32): differs from a
 * BLAS fp32 GEMM by summation order only.
 * ---------------------------------------------------------------------------------- */
int ovis_gemm_f32(const float* A, long a_row_stride, long a_k_stride, const float* B,
                  long b_row_stride, long b_k_stride, const float* bias, float* C,
                  long c_row_stride, int M, int N, int K, void* stream);

/* General form: C = alpha * A.B^T (+ C when accumulate != 0) + bias, bias indexed by column n or, when
 * bias_per_row != 0, by row m (convolution bias in the deformable-conv products). */
int ovis_gemm_ex_f32(const float* A, long a_row_stride, long a_k_stride, const float* B,
                     long b_row_stride, long b_k_stride, const float* bias, int bias_per_row,
                     float alpha, int accumulate, float* C, long c_row_stride, int M, int N, int K,
                     void* stream);

/* The same product with K cut into slices when the problem has too few tiles to fill the chip (the head's small
 * GEMMs: a weight gradient contracts over ~1000 rows into a 768 x 2048 result): every slice writes its own fp32 slab
 * in `workspace` and one kernel adds the slabs in slice order -- no atomics, bit-reproducible run to run.
 * ovis_gemm_f32_workspace_bytes(M, N, K) = bytes the split needs (0: the problem is not cut); workspace NULL = never
 * cut (what ovis_gemm_f32 / ovis_gemm_ex_f32 do); too small a workspace: OVIS_ENOSPC. */
size_t ovis_gemm_f32_workspace_bytes(int M, int N, int K);
int ovis_gemm_ex_ws_f32(const float* A, long a_row_stride, long a_k_stride, const float* B,
                        long b_row_stride, long b_k_stride, const float* bias, int bias_per_row,
                        float alpha, int accumulate, float* C, long c_row_stride, int M, int N, int K,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Region <-> noun alignment of the teacher (mb/modeling/detector/st_generalized_rcnn.py:243-262):
 * for every noun w: raw_scores[w] = max_p <region_emb[p], noun_emb[w]>, best_region[w] = argmax_p
 * (lowest p on exact ties), sigmoid_scores[w] = sigmoid(raw).  region_emb [num_regions, dim],
 * noun_emb [num_nouns, dim]; the [num_regions, num_nouns] score matrix is never materialised. */
int ovis_region_noun_align_f32(const float* region_emb, const float* noun_emb, float* raw_scores,
                               float* sigmoid_scores, int64_t* best_region, int num_regions,
                               int num_nouns, int dim, void* stream);

/* ------------------------------------------------------------------------------------
 * Student losses, forward + backward fused
 *   weighted CE : mb/modeling/roi_heads/box_head/loss.py:172-174
 *     loss[0] = sum_p w[label_p] * CE(logits_p, label_p) / num_rows, w[0] = bg_weight, w[c>0] = 1;
 *     dlogits (may be NULL) receives d loss / d logits.  row_scratch: num_rows floats.
 *   stochastic mask BCE : mb/modeling/roi_heads/mask_head/roi_mask_predictors.py:41-65,
 *                         mb/modeling/roi_heads/mask_head/loss.py:117-148
 *     z = mu + eps * sigma on logit channel `channel` of the positive RoIs pos_index[0..num_pos);
 *     loss[0] = mean BCEWithLogits(z, targets); dmu [num_rois, C, pixels] and dsigma [num_rois, pixels]
 *     (either may be NULL) are fully written (zero outside the positives).  sigma / eps may be NULL
 *     (plain BCE).  mu [num_rois, C, pixels], sigma [num_rois, pixels], eps [num_rois, C, pixels],
 *     targets [num_pos, pixels].  row_scratch: num_pos floats.
 *     `_classes_`: the logit channel of positive i is channels[i] (class-specific masks,
 *     CLS_AGNOSTIC_MASK False: mask_logits[positive_inds, labels_pos], mask_head/loss.py:131-141;
 *     values outside [0, C) are clamped); eps, when given, is read at the same channel.
 * ---------------------------------------------------------------------------------- */
int ovis_weighted_ce_fwd_bwd_f32(const float* logits, const int64_t* labels, float bg_weight,
                                 float* loss, float* dlogits, float* row_scratch, int num_rows,
                                 int num_classes, void* stream);
int ovis_mask_bce_stochastic_fwd_bwd_f32(const float* mu, const float* sigma, const float* eps,
                                         const int64_t* pos_index, const float* targets, float* loss,
                                         float* dmu, float* dsigma, float* row_scratch, int num_rois,
                                         int num_pos, int num_channels, int mask_pixels, int channel,
                                         void* stream);
int ovis_mask_bce_stochastic_classes_fwd_bwd_f32(const float* mu, const float* sigma, const float* eps,
                                                 const int64_t* pos_index, const int64_t* channels,
                                                 const float* targets, float* loss, float* dmu, float* dsigma,
                                                 float* row_scratch, int num_rois, int num_pos,
                                                 int num_channels, int mask_pixels, void* stream);

/* ------------------------------------------------------------------------------------
 * Deformable convolution v1 / v2 building blocks      mb/csrc/deform_conv.h:11-190
 *   kernels: mb/csrc/cuda/deform_conv_kernel_cuda.cu:198-250 (im2col), :287-342 (col2im),
 *            :381-443 (col2im_coord), modulated variants :578-774; host loops deform_conv_cuda.cu:161-694
 * columns [channels*kernel_h*kernel_w, num_images, H_out, W_out]; input [num_images, channels, H, W];
 * offset [num_images, deformable_group*2*kernel_h*kernel_w, H_out, W_out];
 * mask   [num_images, deformable_group*kernel_h*kernel_w, H_out, W_out] or NULL (v1).
 * col2im ACCUMULATES into grad_input (caller zero-fills, as the reference does); col2im_coord overwrites
 * grad_offset (and grad_mask when non-NULL).  The surrounding GEMMs are ovis_gemm_ex_f32 on this layout.
 * ---------------------------------------------------------------------------------- */
int ovis_deform_im2col_f32(const float* input, const float* offset, const float* mask, float* columns,
                           int num_images, int channels, int height, int width, int kernel_h,
                           int kernel_w, int pad_h, int pad_w, int stride_h, int stride_w,
                           int dilation_h, int dilation_w, int deformable_group, void* stream);
int ovis_deform_col2im_f32(const float* columns, const float* offset, const float* mask,
                           float* grad_input, int num_images, int channels, int height, int width,
                           int kernel_h, int kernel_w, int pad_h, int pad_w, int stride_h,
                           int stride_w, int dilation_h, int dilation_w, int deformable_group,
                           void* stream);
int ovis_deform_col2im_coord_f32(const float* columns, const float* input, const float* offset,
                                 const float* mask, float* grad_offset, float* grad_mask,
                                 int num_images, int channels, int height, int width, int kernel_h,
                                 int kernel_w, int pad_h, int pad_w, int stride_h, int stride_w,
                                 int dilation_h, int dilation_w, int deformable_group, void* stream);

/* Deformable convolution forward WITHOUT the column buffer (mb/csrc/cuda/deform_conv_cuda.cu:161-260, :491-560;
 * sampling: deform_conv_kernel_cuda.cu:198-250, 578-644): one implicit GEMM over rows = output pixels (batch, out_h,
 * out_w) and K = (tap, channel) on the pair-layout split GEMM of the res5 head -- the A tile of every k-step is bilinear-
 * sampled in the kernel (zero padding, the reference's four-term order, times the mask when given) from input_nhwc
 * [batch, height, width, channels] fp32, split into bf16 hi / lo and multiplied with weight_pair [out_channels,
 * taps * channels] (tap-major pair rows: ovis_weight_prep_pair_f32).  offset [batch, dg*2*taps, out_h, out_w], mask
 * [batch, dg*taps, out_h, out_w] or NULL (v1), bias [out_channels] or NULL; output [batch*out_h*out_w, out_channels]
 * fp32 rows (NHWC), row stride ldc.  Convolution groups = 1; (channels / deformable_group) % 32 == 0,
 * out_channels % 4 == 0 (else OVIS_ERANGE: use the column route). */
int ovis_deform_conv_implicit_f32(const float* input_nhwc, const float* offset, const float* mask,
                                  const void* weight_pair, long weight_row_bytes, const float* bias, float* output,
                                  long ldc, int batch, int channels, int height, int width, int out_channels, int out_h,
                                  int out_w, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h,
                                  int pad_w, int dil_h, int dil_w, int deformable_group, void* stream);

/* Text side of the cross-modal head: mb/modeling/language_backbone/transformers.py:27-68 (BERT.forward: the frozen
 * word-embedding table indexed by the token ids, no transformer forward) + mb/modeling/detector/st_generalized_rcnn.py:
 * 202-209 (extract_emb): out[n] = normalize( sum_l (1 - special[n,l]) * table[ids[n,l]] / sum_l (1 - special[n,l]) ),
 * normalize = x / max(||x||_2, 1e-12).  table [table_rows, dim] f32 (dim % 4 == 0), input_ids / special_tokens_mask
 * [num_words, max_tokens] int32 as the tokenizer pads them ([CLS], [SEP], [PAD] carry special = 1), out [num_words,
 * dim].  The [num_words, max_tokens, dim] tensor the reference builds is never materialised.  A token id outside the
 * table makes that word's row NaN. */
int ovis_text_embed_f32(const float* table, long table_rows, int dim, const int32_t* input_ids,
                        const int32_t* special_tokens_mask, int num_words, int max_tokens, float* out, void* stream);

/* Polygon ground truth -> mask-head targets: project_masks_on_boxes (mb/modeling/roi_heads/mask_head/loss.py:11-42)
 * for SegmentationMask(mode='poly') targets -- PolygonInstance.crop / resize / convert_to_binarymask
 * (mb/structures/segmentation_mask.py:270-334), whose rasteriser is pycocotools' rleFrPoly + merge + decode
 * (pycocotools==2.0, requirements.txt:35; restated, see csrc/polygons.hip).  coords: all polygons' (x, y) float32
 * pairs back to back; polygon q owns coords[polygon_start[q] .. polygon_start[q+1]) (offsets in floats, even);
 * ground-truth instance g owns polygons [instance_start[g], instance_start[g+1]) (polygons with < 3 vertices are
 * skipped, as PolygonInstance.__init__ drops them); gt_index [num] int64 picks the instance of every box; boxes
 * [num, 4] xyxy in image pixels; out [num, resolution, resolution] f32 in {0, 1}.  resolution <= 64. */
int ovis_project_polygon_masks_f32(const float* coords, const int32_t* polygon_start, const int32_t* instance_start,
                                   const int64_t* gt_index, const float* boxes, int num, int image_width,
                                   int image_height, int resolution, float* out, void* stream);

/* Whole-image masks of polygon instances: SegmentationMask(mode='poly').convert('mask') (mb/structures/
 * segmentation_mask.py:326-334: frPyObjects -> merge -> decode at the image size, no crop / resize), the device twin of
 * ovis_cpu_polygons_to_masks_u8 (include/ovis_cpu.h) with the polygon layout of ovis_project_polygon_masks_f32; any canvas
 * with width * height <= 2^30.  num_polygons = entries of polygon_start - 1.  out [num_instances, height, width] uint8 in
 * {0, 1}, every byte written.  workspace: ovis_polygons_to_masks_workspace_bytes(num_polygons, width, height) bytes,
 * 16-byte aligned (one bit per position and polygon; may be NULL when num_polygons == 0); too small: OVIS_ENOSPC.
 * Enqueues a memset and four kernels on `stream`; xor toggles and a parity scan, so the result is order independent. */
size_t ovis_polygons_to_masks_workspace_bytes(int num_polygons, int width, int height);
int ovis_polygons_to_masks_u8(const float* coords, const int32_t* polygon_start, const int32_t* instance_start,
                              int num_instances, int num_polygons, int width, int height, void* workspace,
                              size_t workspace_bytes, uint8_t* out, void* stream);

/* The input transform: B raw RGB images -> the padded batch the step reads, what the reference does per image on the host
 * (mb/data/transforms/transforms.py:27-62 Resize = PIL Image.resize(BILINEAR), :65-85 RandomHorizontalFlip / VerticalFlip,
 * :105-120 ToTensor + Normalize; mb/structures/image_list.py:29-70 zero padding), bit for bit (csrc/resample_geom.h, shared
 * with the host twin ovis_cpu_transform_images_u8).  data: `data_bytes` bytes holding the images HWC uint8 back to back;
 * desc [batch, 7] int32 ON THE DEVICE = (byte offset, in_h, in_w, out_h, out_w, flip_h, flip_v) per image, never read back;
 * mean[3], std[3] HOST arrays in output-channel order (INPUT.PIXEL_MEAN / PIXEL_STD); to_bgr255: channels reversed and
 * left at 0..255, else RGB / 255.  out [batch, 3, pad_h, pad_w] f32: EVERY element is written exactly once, the zeros
 * right of out_w and below out_h included, so out needs no fill.  max_in_h / max_in_w bound the descriptors' in_h /
 * in_w (they size the first launch and the workspace); an image whose descriptor breaks a bound, the canvas or the byte
 * buffer comes out as NaN and nothing outside the buffers is touched.  workspace:
 * ovis_transform_images_workspace_bytes(batch, max_in_h, pad_w) bytes (the 8-bit image between PIL's two passes); too
 * small: OVIS_ENOSPC.  Two launches whatever the batch, enqueue only.  Any of max_in_h, max_in_w, pad_h, pad_w above
 * 16384 or batch above 65535: OVIS_ERANGE. */
size_t ovis_transform_images_workspace_bytes(int batch, int max_in_h, int pad_w);
int ovis_transform_images_u8(const uint8_t* data, long data_bytes, const int32_t* desc, int batch, int max_in_h,
                             int max_in_w, const float* mean, const float* std, int to_bgr255, int pad_h, int pad_w,
                             void* workspace, size_t workspace_bytes, float* out, void* stream);

/* The input transform with scale jitter and a fixed-size crop (large-scale jitter): a random scale, then a crop or pad to a
 * fixed canvas.  THE RULE is Detectron2's ResizeScale + FixedSizeCrop restated; Detectron2 was not run against it.
 * Parameters: a scale range (lo, hi), 0 < lo <= hi, and a canvas (crop_h, crop_w), default 1024 x 1024.  Per image, drawn
 * on Python's random.Random in the loader worker (data/transforms.py::InputTransform.host), behind the colour-jitter draws
 * when those are on:
 *   1. s = rng.uniform(lo, hi), IN PLACE OF the choice among INPUT.MIN_SIZE_TRAIN (not read in this mode, nor is
 *      MAX_SIZE_TRAIN).  r = min(crop_h * s / in_h, crop_w * s / in_w); out_h = max(1, round(in_h * r)),
 *      out_w = max(1, round(in_w * r)); Python doubles, Python's round (half to even).
 *   2. the two flip draws, as without the jitter.
 *   3. the crop window, in the frame of the resized, FLIPPED image: fy = rng.random(), fx = rng.random(), always drawn;
 *      win_y = round(fy * max(out_h - crop_h, 0)), win_x = round(fx * max(out_w - crop_w, 0));
 *      win_h = min(crop_h, out_h - win_y), win_w = min(crop_w, out_w - win_x).
 *   4. if the image had at least one ground-truth box and none survives step 5: fy, fx are drawn again and step 3 redone,
 *      at most 8 times; the last draw stands (the image may still arrive without targets).
 *   5. targets: resize and flips as without the jitter, then BoxList.crop((win_x, win_y, win_x + win_w, win_y + win_h))
 *      (mb/structures/bounding_box.py:167-193; fields through their own crop), then clip_to_image(remove_empty=True).
 *      The target's size is (win_w, win_h), the image's size (win_h, win_w).
 * The batch is [batch, 3, pad_h, pad_w], (pad_h, pad_w) the canvas rounded up to DATALOADER.SIZE_DIVISIBILITY, zero outside
 * win_h x win_w.
 *
 * ovis_transform_images_window_u8: the device half.  Everything as ovis_transform_images_u8 except desc [batch, 11] int32 =
 * its seven followed by (win_y, win_x, win_h, win_w); out_h / out_w stay the FULL resized size, which is never
 * materialised and may exceed the canvas (up to 16384).  out element (Y, X) with Y < win_h and X < win_w is the normalised
 * pixel (win_y + Y, win_x + X) of the resized, flipped image -- the arithmetic of csrc/resample_geom.h at the positions of
 * the full resize, 8-bit rounding between the two passes included, so the bits of that window sliced out of
 * ovis_transform_images_u8's output -- and zero elsewhere; every element written once.  The horizontal pass computes only
 * the columns the window shows, over the input rows its rows read.  An image is NaN, every other image untouched, when its
 * descriptor breaks max_in_h / max_in_w, out_h or out_w is above 16384, its window leaves [0, out_h) x [0, out_w), win_h >
 * pad_h or win_w > pad_w, or its bytes leave the buffer.  workspace: ovis_transform_images_window_workspace_bytes(batch,
 * max_in_h, pad_w) = batch * max_in_h * pad_w * 3 bytes, whatever the scale.  Two launches whatever the batch, enqueue only.
 * Host twin: ovis_cpu_transform_images_window_u8. */
size_t ovis_transform_images_window_workspace_bytes(int batch, int max_in_h, int pad_w);
int ovis_transform_images_window_u8(const uint8_t* data, long data_bytes, const int32_t* desc, int batch, int max_in_h,
                                    int max_in_w, const float* mean, const float* std, int to_bgr255, int pad_h, int pad_w,
                                    void* workspace, size_t workspace_bytes, float* out, void* stream);

/* Colour jitter in front of the input transform: ColorJitter, first in the reference's training Compose
 * (mb/data/transforms/build.py:29-45, transforms.py:88-102 = torchvision's, which composes PIL calls), on the packed bytes
 * of ovis_transform_images_u8, with the bytes PIL 12 produces (csrc/color_jitter_chain.h, shared with the host twin
 * ovis_cpu_color_jitter_u8).  The arithmetic was compared with PIL byte for byte; the COMPOSITION of the PIL calls is
 * torchvision 0.4-0.7's functional_pil written out here, not run against torchvision.
 *
 * Per image, on the original RGB image before the resize, the operations of its row of `ops` run in that order, each on
 * the previous one's 8-bit result:
 *   blend(d, x, a), d the degenerate value and x the pixel, 0..255, a the float32 factor:
 *     t = (float)d + a * ((float)x - (float)d), three separate float32 operations, never a fused multiply-add;
 *     0 <= a <= 1: (uint8)t, truncated; otherwise 0 if t <= 0 (or NaN), 255 if t >= 255, else (uint8)t.
 *   grey(r, g, b) = (r*19595 + g*38470 + b*7471 + 0x8000) >> 16.
 *   0 brightness f: every channel blend(0, x, f).
 *   1 contrast f:   m = (int)(S / N + 0.5), S the exact integer sum of grey over the image AS IT IS AT THIS POINT of the
 *                   chain, N its pixels, division and addition in fp64 (greys 10 and 11: m = 11); every channel blend(m, x, f).
 *   2 saturation f: every channel blend(grey(r, g, b), x, f).
 *   3 hue shift s (an integer 0..255 held exactly in the float; anything else shifts by 0): RGB -> HSV, h = (h + s) & 255,
 *                   HSV -> RGB.  The round trip is NOT the identity, so it runs for s == 0 too.
 *     RGB -> HSV: v = max; max == min: h = s = 0.  Otherwise in float32 cr = max - min, sat = cr / max, rc, gc, bc =
 *       (max - r|g|b) / cr; hf = (float)(bc - gc) if r == max, else (float)(2.0 + (double)rc - (double)bc) if g == max, else
 *       (float)(4.0 + (double)gc - (double)rc); hf = (float)fmod((double)hf / 6.0 + 1.0, 1.0);
 *       h = clip8((int)((double)hf * 255.0)); s = clip8((int)(sat * 255.f)).
 *     HSV -> RGB in fp64: s == 0: (v, v, v).  Otherwise hh = h * 6.0 / 255.0, i = floor(hh), f = hh - i, fs = s / 255.0,
 *       p = rnd(v * (1 - fs)), q = rnd(v * (1 - fs * f)), t = rnd(v * (1 - fs * (1 - f))), rnd(x) = clip8(floor(x + 0.5));
 *       (r, g, b) by i % 6: (v,t,p) (q,v,p) (p,v,t) (p,q,v) (t,p,v) (v,p,q).
 *
 * data, data_bytes, desc: as ovis_transform_images_u8; only offset, in_h and in_w of a descriptor are read.  ops [batch, 4]
 * int32: the codes above in application order, -1 for an unused trailing slot; params [batch, 4] f32, slot-aligned: the
 * factor, for hue the shift.  Both ON THE DEVICE, never read back.  out: a second buffer of data_bytes bytes with the same
 * layout; the bytes of every valid image are written, nothing else.  out overlapping data: OVIS_EINVAL (contrast reads the
 * whole image).  An image whose descriptor leaves the byte buffer or max_in_h / max_in_w writes nothing (the transform
 * behind it turns it into NaN); a malformed row of ops (a code outside -1..3, a repeated code, a code behind an unused
 * slot) copies its image unchanged; no table content makes a kernel leave data, out or the workspace.
 * workspace: ovis_color_jitter_workspace_bytes(batch) bytes, 8-byte aligned: one 64-bit grey sum per image, zeroed on the
 * stream; too small: OVIS_ENOSPC.  workspace NULL: the caller states that no row holds contrast -- the sum launch is
 * skipped, and a row that holds contrast anyway copies its image unchanged.  At most two launches whatever the batch,
 * enqueue only; integer sums, so two runs give the same bytes.  max_in_h or max_in_w above 16384, batch above 65535:
 * OVIS_ERANGE. */
size_t ovis_color_jitter_workspace_bytes(int batch);
int ovis_color_jitter_u8(const uint8_t* data, long data_bytes, const int32_t* desc, const int32_t* ops, const float* params,
                         int batch, int max_in_h, int max_in_w, void* workspace, size_t workspace_bytes, uint8_t* out,
                         void* stream);

/* Copy-paste augmentation behind scale jitter (the other half of "Simple Copy-Paste", Ghiasi et al., CVPR 2021): objects of
 * one image of a batch are pasted, at the same canvas position, over another.  THE RULE below is this project's own
 * statement; it was NOT compared with any other implementation's output.
 * Parameter: P in (0, 1] (tools/train_net.py --copy-paste P; needs --scale-jitter, whose fixed canvas gives "the same
 * position in the other image" a meaning and bounds the memory; polygon ground truth only).
 * Host half, on Python's random.Random in the loader worker (data/transforms.py::InputTransform.host), AFTER every image of
 * the batch has made its own draws and has its cropped target -- those draws are exactly a run's without the flag:
 *   - a batch of B < 2 images, or one without targets, makes no copy-paste draw and is handed on unchanged.
 *   - for i = 0 .. B-1 in order the source is j = (i + 1) % B: u = rng.random(); image i receives a paste iff u < P.  Then
 *     one rng.random() per instance of source j's cropped target, in order; an instance is selected iff its draw is < 0.5.
 *     A source without instances, or no selected instance: no paste for i.  Sources are the PRE-paste images and targets.
 *   - a pasted-into image i: its frame is (max(win_h_i, win_h_j), max(win_w_i, win_w_j)) -- both windows start at the canvas
 *     origin --, its boxes and labels are cat(own rows, selected source rows), the source's boxes as they are; every other
 *     field stays i's.  paste_src [B] int32 holds j, or -1.
 * Device half, per image with paste_src >= 0:
 *   1. own and pasted polygons rasterised at the new frame (ovis_polygons_to_masks_u8): uint8 [G_own + G_paste, h, w].
 *   2. alpha = OR of the pasted masks, 0 / 1; every own mask becomes mask & ~alpha, in place.
 *   3. per own mask the int32 row (pixels before, pixels after, x1, y1, x2, y2): the tight box of what is left in pixel
 *      indices (x2 = max x: the TO_REMOVE = 1 convention); an empty remainder is the box (0, 0, -1, -1).
 *   4. the table is read back (the only read-back).  An own instance whose count did not change is untouched: it keeps its
 *      annotation box and stays, even at a count of 0.  A touched one takes the tight box as float32 and stays iff x2 > x1
 *      and y2 > y1 (clip_to_image(remove_empty=True)'s test; no new threshold).  Pasted instances always stay, with their
 *      annotation boxes.  The target's masks are the dense uint8 [G', h, w] rows kept, own first.
 *   5. pixels, on the float batch of ovis_transform_images_window_u8: out[i, c, y, x] = alpha_i[y, x] ? in[paste_src[i], c,
 *      y, x] : in[i, c, y, x], bit-wise, the right-hand side pre-paste for every i.
 *
 * ovis_copy_paste_masks_u8: steps 2 and 3.  masks [num_own + num_paste, height, width] uint8, own first; a byte that is not
 * zero is a set pixel.  alpha_out [height, width] uint8: every byte written, 0 / 1 (all 0 when num_paste == 0; written when
 * num_own == 0 too).  Own masks in place: a covered byte becomes 0, every other byte stays.  stats_out [num_own, 6] int32 as
 * in 3, may be NULL when num_own == 0.  Two launches (one when num_own == 0), one workgroup per own mask, no atomics: the
 * same words on every call.  Enqueue only.  height or width < 1, a negative count, a NULL pointer that is needed:
 * OVIS_EINVAL; height * width > 2^30: OVIS_ERANGE.
 *
 * ovis_copy_paste_images_f32: step 5, IN PLACE on batch [num_images, channels, pad_h, pad_w] f32.  HOST arrays of
 * num_images entries: paste_src (-1: the image receives nothing and its two other entries are not read), alpha_ptrs (DEVICE
 * pointers: the image's alpha) and alpha_hw [num_images, 2] = its alpha's (height, width), at most the canvas'; outside its
 * frame an alpha is 0.  One thread owns a pixel position across the whole batch and loads every pre-paste value before it
 * stores, so swaps and cycles are exact.  One launch, none when no image has a source.  At most
 * OVIS_BOX_DECODE_MAX_IMAGES images (they travel as kernel arguments): above, OVIS_ERANGE and nothing is written.  A
 * source outside [-1, num_images), a frame outside the canvas, a NULL pointer: OVIS_EINVAL. */
int ovis_copy_paste_masks_u8(uint8_t* masks, int num_own, int num_paste, int height, int width, uint8_t* alpha_out,
                             int32_t* stats_out, void* stream);
int ovis_copy_paste_images_f32(float* batch, int num_images, int channels, int pad_h, int pad_w,
                               const uint8_t* const* alpha_ptrs, const int32_t* alpha_hw, const int32_t* paste_src,
                               void* stream);

/* Deformable convolution BACKWARD on NHWC rows (csrc/deform_conv_rows.hip; mb/csrc/cuda/deform_conv_cuda.cu:271-497,
 * 580-694): rows m = (image, h_out, w_out), k = (tap, channel), the layout of ovis_deform_conv_implicit_f32.
 * ovis_deform_im2col_pair_rows_f32: the sampled (x mask) rows col[m, (t, c)] written ONCE, in pair layout (row stride
 *   columns_row_bytes >= 4 * taps * channels) -- the X operand of ovis_split_gemm_pair_tn for the weight gradient.
 * ovis_deform_col2im_rows_f32: one pass over dcol_rows [rows, dcol_ld >= taps * channels] fp32 (= dY . W, an
 *   ovis_split_gemm_pair product): grad_input_nhwc [batch, height, width, channels] += scatter (fp32 atomics; the caller
 *   zero-fills), grad_offset [batch, dg*2*taps, out_h, out_w] and grad_mask [batch, dg*taps, out_h, out_w] += the
 *   coordinate / mask gradients (atomics: the caller zero-fills; grad_mask / mask NULL = v1).  Either output group may be
 *   NULL.  (channels / deformable_group) % 32 == 0, else OVIS_ERANGE. */
int ovis_deform_im2col_pair_rows_f32(const float* input_nhwc, const float* offset, const float* mask, void* columns_pair,
                                     long columns_row_bytes, int batch, int channels, int height, int width, int out_h,
                                     int out_w, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w,
                                     int dil_h, int dil_w, int deformable_group, void* stream);
int ovis_deform_col2im_rows_f32(const float* dcol_rows, long dcol_ld, const float* input_nhwc, const float* offset,
                                const float* mask, float* grad_input_nhwc, float* grad_offset, float* grad_mask, int batch,
                                int channels, int height, int width, int out_h, int out_w, int kernel_h, int kernel_w,
                                int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, int deformable_group,
                                void* stream);

/* Last bottleneck of a res5 chain with the head's average pooling in the GEMM epilogue (mb/modeling/roi_heads/box_head/
 * roi_box_predictors.py:62-66: AdaptiveAvgPool2d over the 7 x 7 map of every RoI): act(A.B^T + bias + shortcut) as
 * ovis_split_gemm_pair_rp, and pooled[m / pool_rows][n] += pool_scale * result summed over the pool_rows rows of every map
 * (32 <= pool_rows <= 64; `pooled` [ceil(m / pool_rows), n] fp32 must be ZERO-FILLED by the caller; every pooled value
 * receives at most two fp32 atomic addends: bit-reproducible).  c and c_pair may BOTH be NULL: then nothing but the pooled
 * rows is written (the no-grad teacher pass).  residual_pair may be NULL.  Plain un-split 128-column launches only:
 * ovis_split_gemm_pair_pool_supported(m, n, channels, pool_rows) != 0, else OVIS_ERANGE. */
int ovis_split_gemm_pair_pool_supported(long m, int n, int channels, int pool_rows);
int ovis_split_gemm_pair_rp_pool(const void* a_pair, long a_row_bytes, const void* b_pair, long b_row_bytes, float* c,
                                 long ldc, void* c_pair, long c_pair_row_bytes, const float* bias,
                                 const void* residual_pair, long residual_pair_row_bytes, long m, int n, int channels,
                                 int relu, float* pooled, int pool_rows, float pool_scale, void* stream);

/* SGD with momentum / weight decay over many tensors in one launch (mb/solver/build.py:8-37 + torch.optim.SGD's update;
 * engine/solver.py): items = device array of {float* p; const float* g; float* buf; long n} (32 bytes each), blocks = device
 * array of int2 (item, chunk): block b updates elements [chunk * ovis_sgd_chunk_elements(), ...) of its item with
 *   d = g + wd * p (when apply_weight_decay);  buf = momentum * buf + d (when momentum != 0);  p += (-lr) * (buf or d)
 * in exactly that fp32 operation order (bit-identical to the six multi-tensor passes it replaces). */
int ovis_sgd_momentum_multi_f32(const void* items, const void* blocks, int num_blocks, float lr, float weight_decay,
                                float momentum, int apply_weight_decay, void* stream);
int ovis_sgd_chunk_elements(void);

/* The same SGD update with an exponential moving average (EMA) of the weights moved in the same pass
 * (engine/ema.py::ModelEma, engine/solver.py::GroupFusedSGD.ema; tools/train_net.py --ema DECAY).  The rule:
 *   - the average covers exactly the parameters with requires_grad (model.named_parameters()), keyed by name, fp32, on the
 *     parameters' device; frozen weights are shared with the live model and FrozenBN has no moving buffers;
 *   - the average e starts as a copy of the parameters when the EMA object is made (behind the load of MODEL.WEIGHT), the
 *     update count at t = 0;
 *   - at every optimizer step, behind the SGD update of an element:  d_t = min(DECAY, (1 + t) / (10 + t)) in Python doubles,
 *     w = float32(1 - d_t), and in fp32 without contraction, three separate roundings:
 *         diff = p_new - e;   e = e + diff * w
 *     then t += 1, once per optimizer step (with SOLVER.GRADIENT_ACCUMULATION_STEPS > 1 only when the optimizer steps);
 *   - a parameter the step skips (p.grad is None) gets no EMA update in that step: the EMA update covers exactly the
 *     elements the SGD update covers (t still advances: it counts optimizer steps);
 *   - every rank keeps its own average; they are equal by construction, so there is no collective.
 * items = device array of {float* p; const float* g; float* buf; float* ema; long n} (40 bytes each); blocks, chunking and
 * the SGD operation sequence are those of ovis_sgd_momentum_multi_f32, so p and buf are bit-identical to it; the EMA lines
 * are applied to the p just computed, from registers (p, g, buf, ema read, buf, p, ema written once: 28 bytes per element
 * against 20).  ema_weight = w.  No atomics: every element is written once.  p, buf, ema must not overlap. */
int ovis_sgd_momentum_ema_multi_f32(const void* items, const void* blocks, int num_blocks, float lr, float weight_decay,
                                    float momentum, int apply_weight_decay, float ema_weight, void* stream);

/* a[i] <-> b[i] over many tensors in one launch, bit-wise (32-bit words: NaN payloads, signed zeros and subnormals are
 * exchanged untouched) and in place: items = device array of {void* a; void* b; long n} (24 bytes each, n in 4-byte
 * elements, a and b disjoint), blocks as above.  How the averaged weights are put into a model and taken out again
 * (ModelEma.applied): values move, pointers stay -- the optimizer's tables, the reducer's gradient views, the momentum
 * buffers and every Parameter object stay valid, and two swaps restore every bit.  Evaluations of the averaged weights write
 * under OUTPUT_DIR/inference_ema/, those of the raw weights under OUTPUT_DIR/inference/. */
int ovis_swap_multi_f32(const void* items, const void* blocks, int num_blocks, void* stream);

/* The backward of an identity bottleneck (mb/modeling/backbone/resnet.py:290-342: out = relu(conv3(relu(conv2(relu(conv1(x)))))
 * + x); autograd derives the backward) inside a pair-only chain, behind ONE call: g3 [m, channels] = the gradient w.r.t. the
 * block's output, already gated and in pair layout (what ovis_split_gemm_pair_rp_gated of the block above wrote); x / o1 / o2 =
 * the block's input and its conv1 / conv2 outputs (post-ReLU) in pair layout; t1 [channels, mid], t2 [mid, taps * mid],
 * t3 [mid, channels] = the transposed pair forms of the folded weights (ovis_weight_prep_pair_f32's second result);
 * scale1..3 = the folded FrozenBN scales the raw weights' gradients are multiplied with (NULL: none).  Writes
 *   g2 [m, mid], g1 [m, mid] (pair), gx [m, channels] (pair: the gated gradient for the block below),
 *   dw1 [mid, channels, 1, 1], dw2 [mid, mid, taps_h, taps_w], dw3 [channels, mid, 1, 1] (fp32)
 * by exactly the launches the separate entry points make (ovis_split_gemm_pair_gated_ws x 2, ovis_split_gemm_pair_rp_gated,
 * ovis_split_gemm_pair_tn + ovis_slab_reduce_f32 x 3: bit-identical results), the data-gradient chain on `stream`, the three
 * weight gradients on `side_stream` (NULL = `stream`) ordered against the chain by events; `stream` waits for them before
 * whatever the caller enqueues next.  channels % 128 == 0, mid_channels % 128 == 0, odd taps. */
size_t ovis_bottleneck_identity_backward_workspace_bytes(long m, int channels, int mid_channels, int taps_h, int taps_w,
                                                         int width, int config);
int ovis_bottleneck_identity_backward(
    const void* g3_pair, long g3_row_bytes, const void* x_pair, long x_row_bytes, const void* o1_pair, long o1_row_bytes,
    const void* o2_pair, long o2_row_bytes, const void* t1_pair, long t1_row_bytes, const void* t2_pair, long t2_row_bytes,
    const void* t3_pair, long t3_row_bytes, const float* scale1, const float* scale2, const float* scale3, long m, int channels,
    int mid_channels, int taps_h, int taps_w, int height, int width, void* g2_pair, void* g1_pair, void* gx_pair, float* dw1,
    float* dw2, float* dw3, void* workspace, size_t workspace_bytes, int config, void* stream, void* side_stream);

/* Weight preparation of MANY convolutions in one launch, behind the optimizer step (mb/engine/trainer.py:139; what
 * ovis_weight_prep_pair_f32 does per convolution): items = device array of 64-byte records
 *   {const float* w [N, C, T]; const float* scale [N] or NULL; void* fwd; void* bwd or NULL; long fwd_row_bytes;
 *    long bwd_row_bytes; int N, C, T, pad}
 * (fwd row n at fwd + n * fwd_row_bytes holds the pair form of w[n, :, :] * scale[n] tap-major, k = t * C + c; bwd row c at
 * bwd + c * bwd_row_bytes the transposed matrix, k' = t * N + n; a row stride above 4 * T * C writes into a wider matrix:
 * [w3 | wd] of a projection block), blocks = device array of int2 (item, tile): workgroup b converts tile (tile / (C / 32),
 * tile % (C / 32)) of 32 output x 32 input channels (ovis_weight_prep_tile() = 32) of its item, all T taps; an item has
 * (N / 32) * (C / 32) tiles.  max_taps = the largest T in the table (<= 15: the tile is staged in LDS).  N % 32 == 0,
 * C % 32 == 0, buffers 16-byte aligned: the CALLER checks (the table is opaque here).  Bit-identical to the per-convolution
 * entry. */
int ovis_weight_prep_pair_multi_f32(const void* items, const void* blocks, int num_blocks, int max_taps, void* stream);
int ovis_weight_prep_tile(void);

/* COCO box / mask AP scoring (csrc/coco_eval.hip): the device half of pycocotools' COCOeval, which the reference calls in
 * mb/data/datasets/evaluation/coco/coco_eval.py:315-333 on the results of :71-162.  A chunk of images is scored at once.
 * A PROBLEM is one (image, category) pair with a detection or a ground truth; `problems` is a device table
 *   int64 [num_problems, 8] = (det_start, det_count, gt_start, gt_count, iou_offset, det_word_start, gt_word_start,
 *                              words_per_mask)
 * over the chunk's detection rows (inside a problem: descending score, stable, at most 100 -- COCOeval.evaluateImg's
 * order), its ground-truth rows (annotation order) and one flat fp64 IoU buffer that holds every problem's
 * [det_count, gt_count] block at iou_offset.  The last three columns are read by the mask IoU only: offsets in 64-bit
 * words into det_words / gt_words and the words of one mask of that image.  The kernels do not check the table; the
 * caller checks it against the buffer sizes on the host.  max_pairs / max_gts: the largest det_count * gt_count /
 * gt_count of the table (they size the grid; max_gts > 4096: OVIS_ERANGE).  Empty inputs return before any launch.
 *
 * ovis_coco_box_iou_f64 (COCOeval.computeIoU, iouType bbox; coco_eval.py:71-105 makes the xywh boxes): dets / gts fp64
 *   xywh rows;  iw = min(dx+dw, gx+gw) - max(dx, gx) clamped at 0, ih likewise, i = iw*ih,
 *   u = crowd ? dw*dh : dw*dh + gw*gh - i, iou = i / u in exactly this fp64 operation order (no contraction);
 *   u == 0 gives 0 (stated deviation: pycocotools yields NaN).
 * ovis_coco_pack_masks_u64: masks [num, pixels] bytes (the outputs of ovis_paste_masks_u8 / ovis_polygons_to_masks_u8:
 *   coco_eval.py:108-162 pastes with Masker(0.5, padding=1)) -> words [num, ceil(pixels / 64)], pixel p = bit p % 64 of
 *   word p / 64, the tail zero-filled, and areas [num] = the number of set pixels (the `area` of a segm result).
 * ovis_coco_mask_iou_f64 (computeIoU, iouType segm): i = popcount(D & G) as an integer,
 *   u = crowd ? |D| : |D| + |G| - i, iou = double(i) / double(u), u == 0 gives 0: exact.
 * ovis_coco_match (COCOeval.evaluateImg): for every problem, each of num_areas area ranges [lo, hi] (area_ranges
 *   [num_areas, 2] fp64) and each of num_thresholds IoU thresholds (fp64): a ground truth is ignored if it is a crowd or
 *   its area is < lo or > hi; the detections, in row order, each take -- among the ground truths not yet matched at this
 *   threshold and not ignored, with iou >= min(t, 1 - 1e-10) -- the one of largest IoU, ties to the later one; when there
 *   is none, the same among the ignored ones that are unmatched or crowd.  Writes dt_match [num_areas, num_thresholds,
 *   num_dets] int32 = the matched ground truth's index INSIDE its problem (annotation order) or -1, dt_ignore (same
 *   shape, u8) = the matched ground truth's ignore flag, or for an unmatched detection whether its own area is outside
 *   [lo, hi], and gt_ignore [num_areas, num_gts] u8.  Every row that belongs to a problem is written; deterministic, no
 *   atomics.  det_areas / gt_areas fp64, gt_crowd u8.  iou may be NULL when no problem of the table has both a detection
 *   and a ground truth (the IoU buffer is empty then and is not read). */
int ovis_coco_box_iou_f64(const double* dets, const double* gts, const uint8_t* gt_crowd, const int64_t* problems,
                          int num_problems, long max_pairs, double* iou, void* stream);
int ovis_coco_pack_masks_u64(const uint8_t* masks, int num, long pixels, uint64_t* words, int64_t* areas, void* stream);
int ovis_coco_mask_iou_f64(const uint64_t* det_words, const int64_t* det_areas, const uint64_t* gt_words,
                           const int64_t* gt_areas, const uint8_t* gt_crowd, const int64_t* problems, int num_problems,
                           long max_pairs, double* iou, void* stream);
int ovis_coco_match(const double* iou, const int64_t* problems, int num_problems, int max_gts, const double* det_areas,
                    const double* gt_areas, const uint8_t* gt_crowd, const double* area_ranges, int num_areas,
                    const double* thresholds, int num_thresholds, long num_dets, long num_gts, int32_t* dt_match,
                    uint8_t* dt_ignore, uint8_t* gt_ignore, void* stream);

/* Boundary IoU for Boundary AP (csrc/coco_boundary.hip; Cheng et al., "Boundary IoU", CVPR 2021 -- the reference does not
 * score it; neither pycocotools nor boundary-iou-api is a dependency, so the rule is restated and THIS TEXT is the
 * contract).  For a binary mask m of a height x width image:
 *   1. d = max(1, int(round(0.02 * sqrt(height^2 + width^2)))), Python 3's round (half to even), computed by the CALLER
 *      and passed as `dilation` (15x20: 1, 45x60: 2, 75x100: 2, 70x129: 3, 480x640: 16, 800x1333: 31, 1x1: 1).
 *   2. eroded(m) = d iterations of a 3x3 erosion with everything outside the image counted as 0 (mask_to_boundary's
 *      one-pixel zero border and cv2.erode(iterations = d)): pixel (y, x) survives iff y - d >= 0, y + d < height,
 *      x - d >= 0, x + d < width and all (2d + 1)^2 pixels of the square around it are set.
 *   3. boundary(m) = m & ~eroded(m): a mask the image border cuts off has boundary along the border.
 *   4. boundary_iou(D, G) = |b(D) & b(G)| / |b(D) | b(G)|, for a crowd G over |b(D)| -- ovis_coco_mask_iou_f64's forms on
 *      the boundary words, a zero denominator gives 0 -- and the IoU that is matched is min(mask_iou, boundary_iou),
 *      for crowds too.  Areas (the area ranges of ovis_coco_match) stay the MASK areas.
 * ovis_coco_boundary_words_u64: words [num, ceil(height * width / 64)] in ovis_coco_pack_masks_u64's layout (tail bits
 *   zero), all masks of one image size -> boundary_words (same shape; every word is written, tail bits zero) and
 *   boundary_areas [num] = their set bits.  scratch: num * ceil(height * width / 64) words the call may overwrite (the
 *   row-eroded words).  Three launches per 65535 masks, enqueue only, vector loads and stores, no atomics, no host read:
 *   the same bits on every call.  Any dilation >= 1 is served (2 * dilation + 1 > 64, and dilation >= min(height, width)
 *   / 2, where nothing survives and the boundary is the mask).  OVIS_EINVAL: num < 0, height < 1, width < 1,
 *   dilation < 1, a null pointer with num > 0; OVIS_ERANGE: height * width > 0x7fffffef (the encoder's pixel bound);
 *   num == 0: OVIS_OK without a launch.
 * ovis_coco_boundary_iou_f64: ovis_coco_mask_iou_f64 with the boundary words / areas of both sides beside the mask
 *   words / areas (the same `problems` table addresses both word buffers of a side): writes min(mask_iou, boundary_iou)
 *   to the flat IoU buffer ovis_coco_match consumes.  Both ratios are integer / integer converted to fp64: exact. */
int ovis_coco_boundary_words_u64(const uint64_t* words, int num, int height, int width, int dilation, uint64_t* scratch,
                                 uint64_t* boundary_words, int64_t* boundary_areas, void* stream);
int ovis_coco_boundary_iou_f64(const uint64_t* det_words, const uint64_t* det_boundary_words, const int64_t* det_areas,
                               const int64_t* det_boundary_areas, const uint64_t* gt_words,
                               const uint64_t* gt_boundary_words, const int64_t* gt_areas,
                               const int64_t* gt_boundary_areas, const uint8_t* gt_crowd, const int64_t* problems,
                               int num_problems, long max_pairs, double* iou, void* stream);

/* LVIS-style federated AP -- APr / APc / APf (csrc/lvis_eval.hip, engine/coco_eval.py rules="lvis"; Gupta et al., "LVIS",
 * CVPR 2019 -- the reference does not score it).  lvis-api is not a dependency: the rules are restated and THIS TEXT is the
 * contract; the numbers follow it and have NOT been compared with lvis-api's own output.  "COCO's" below means what
 * engine/coco_eval.py and csrc/coco_eval.hip do under rules="coco".
 *   1. SCOPE.  All images and all categories of the annotation file, sorted by id.  Every image must carry
 *      neg_category_ids and not_exhaustive_category_ids (lists of category ids) and every category frequency in {r, c, f};
 *      a missing key is a ValueError naming the first offending image or category -- never silently empty.
 *   2. GROUND TRUTH.  Every annotation is ground truth.  iscrowd is not read: no ground truth is a crowd and no IoU uses the
 *      crowd form.  A ground truth's input ignore flag is its `ignore` key if present, else 0.  Its area is COCO's: `area`
 *      if present, else the box w * h.
 *   3. CAP PER IMAGE, before anything else: an image's detections are sorted by descending score, stably (ties keep
 *      prediction or file order), and the first max_dets = 300 are kept across all categories together.  No per-category
 *      cap of 100.  (Python keyword lvis_max_dets = 300; negative: no cap.)
 *   4. FEDERATED FILTER, after the cap: a kept detection of category c in image i is dropped unless c is in
 *      neg_category_ids(i) or image i has at least one ground truth of c.
 *   5. PROBLEMS.  A problem is an (image, category) pair with a surviving detection or a ground truth; inside it the
 *      detections are ordered by descending score, stably, the ground truths in annotation order.
 *   6. IOU.  COCO's non-crowd form for bbox and segm; for boundary min(mask IoU, boundary IoU) with the dilation rule
 *      above, non-crowd form.  A zero union gives 0 (the stated deviation).
 *   7. MATCHING, one per problem, area range and IoU threshold (COCO's four ranges and ten thresholds).  A ground truth is
 *      ignored in area range a if its input ignore flag is set or its area lies outside the range.  Ground truths are
 *      scanned non-ignored first, in stable order; detections are taken in score order.  A detection takes, among the
 *      UNMATCHED ground truths with IoU >= min(t, 1 - 1e-10), the non-ignored one of largest IoU, an equal IoU going to
 *      the later ground truth; failing a non-ignored match, the same among the ignored ones.  A matched ground truth is
 *      never matched again, ignored or not (the one difference from COCO's loop, where a crowd can be re-matched).  A
 *      detection matched to an ignored ground truth is ignored.
 *   8. UNMATCHED DETECTIONS.  Ignored if the detection's area lies outside the range OR its category is in
 *      not_exhaustive_category_ids of its image.  Area: box w * h for bbox, the mask pixel count for segm and boundary.
 *   9. ACCUMULATE, per category and area range over all images: detections merged by descending score with a stable
 *      (merge) sort in image-id order; tp / fp cumulative sums over the non-ignored detections; precision = tp / (tp + fp +
 *      spacing(1)), made non-increasing from the right, sampled at the 101 recall thresholds by searchsorted(side = left),
 *      recall points past the last detection get 0; recall[t, k, a] = the last tp / num_gt, 0 with no detections.  A
 *      (category, area) with no non-ignored ground truth stays -1.  There is no maxDets dimension.
 *  10. SUMMARISE.  The mean over entries > -1, -1 if there are none: AP, AP50, AP75, APs, APm, APl, then APr, APc, APf
 *      (area "all", restricted to the categories of that frequency), then the project's AP50_class_<name> and
 *      AP50_split_<split>; with recall AR@300, ARs@300, ARm@300, ARl@300 and AR@300_split_<split>.  Fractions.
 * Out of scope: a comparison with lvis-api; LVIS's "fixed AP" variant (10 000 detections per class); a federated training
 * loss; another cap from the command line; keypoints; host-only scoring.
 *
 * ovis_lvis_match (rules 7 and 8): ovis_coco_match's inputs, tables and outputs with two changes -- gt_ignore_in u8
 *   [num_gts] (rule 2's input ignore flag) takes the place of gt_crowd and a matched ground truth is never matched again;
 *   problem_not_exhaustive u8 [num_problems], one flag per row of `problems`, is ORed into the ignore flag of that
 *   problem's unmatched detections.  A problem without ground truth reads no IoU and shuffles nothing: its detections are
 *   written lane-parallel as -1 / (area outside the range | problem flag).  With all-zero gt_ignore_in and flags the output
 *   equals ovis_coco_match's with all-zero gt_crowd, bit for bit.  max_gts > 4096: OVIS_ERANGE; null and zero-size handling
 *   as ovis_coco_match (problem_not_exhaustive must not be NULL when num_problems > 0); iou may be NULL when no pair exists.
 *   Deterministic, no atomics, no LDS. */
int ovis_lvis_match(const double* iou, const int64_t* problems, int num_problems, int max_gts, const double* det_areas,
                    const double* gt_areas, const uint8_t* gt_ignore_in, const uint8_t* problem_not_exhaustive,
                    const double* area_ranges, int num_areas, const double* thresholds, int num_thresholds, long num_dets,
                    long num_gts, int32_t* dt_match, uint8_t* dt_ignore, uint8_t* gt_ignore, void* stream);

/* Error analysis -- AP50 broken down by error type (csrc/error_types.hip, engine/error_analysis.py; Bolya et al., "TIDE: A
 * General Toolbox for Identifying Object Detection Errors", ECCV 2020 -- the reference does not do it).  tidecv is not a
 * dependency: the rules are restated and THIS TEXT is the contract; the numbers follow it and have NOT been compared with
 * tidecv's own output.
 *   SCOPE.  COCO rules only: area range "all", 100 detections per category and image, bbox and segm.  Thresholds t_f = 0.5
 *     (foreground) and t_b = 0.1 (background), compared in fp64; keywords of the Python functions, no command-line switch.
 *   BASE.  The existing matching at (area all, IoU 0.5): dt_match[0, 0], dt_ignore[0, 0] and gt_ignore[0].  A detection is
 *     a false positive when it is unmatched; under area "all" an unmatched detection is never ignored.  A detection
 *     matched to a crowd is ignored and is not an error.  Crowd ground truths take no part in what follows.
 *   IMAGE IOU.  For every image the IoU of all its detection rows against all its ground-truth rows: box IoU for bbox,
 *     mask IoU on the packed words for segm.  Only entries against non-crowd ground truths are read, so the non-crowd form
 *     is all that matters.  For a false positive d of category c, s is the largest IoU over the non-crowd ground truths
 *     of category c and g_s that ground truth; o and g_o are the same over the non-crowd ground truths of every other
 *     category.  A maximum over an empty set is 0 with target -1.  An equal IoU goes to the later ground-truth row (the
 *     project's tie rule everywhere else).
 *   TYPES.  The first rule that holds applies:
 *     1. Loc:  t_b <= s < t_f, target g_s.  Right class, badly localised.
 *     2. Cls:  o >= t_f, target g_o.  Well localised, wrong class.
 *     3. Dupe: s >= t_f, target g_s.  Every such ground truth was taken by a better-scoring detection.
 *     4. Bkg:  max(s, o) <= t_b.
 *     5. Both: everything else.  Wrong class and badly localised.
 *   MISSED.  A non-crowd ground truth is Miss when no detection is matched to it in the base and it is the target of no
 *     Loc or Cls error.
 *   FIXES, each applied alone.  Dupe, Bkg, Both: those detections are deleted.  Loc: the detection becomes a true positive
 *     of its target if the target is free, otherwise it is deleted.  Cls: the detection moves, with its score, into the
 *     target's category; it becomes a true positive there if the target is free, otherwise it is deleted.  Free means
 *     unmatched in the base and not yet claimed in this pass; among fixed detections with the same target the one with
 *     the highest score claims it, ties going to the earlier detection row.  Miss: the missed ground truths are removed,
 *     with their count.  FalsePos: every false positive is deleted.  FalseNeg: every unmatched non-crowd ground truth is
 *     removed.
 *   DAP.  dAP50_<T> is the AP50 after fix T minus the base AP50.  AP50 is the scorer's own: descending score, stable,
 *     merged in image-id order (the detection rows' order: image, category index, descending score; a moved detection
 *     keeps its row), tp / (tp + fp + spacing(1)), the envelope from the right, 101 recall samples, the mean over the
 *     categories with at least one ground truth left.  A category left without ground truth by a fix drops out of that
 *     mean.  If no category remains, or the base is -1, the dAP is -1.  dAP50_<T>_split_<split> is the same with both means
 *     restricted to the categories of a split.
 * Out of scope: LVIS rules, Boundary IoU, other thresholds from the command line, TIDE's plots, host-only analysis.
 *
 * ovis_error_types (IMAGE IOU's maxima, TYPES and MISSED for one chunk of images):
 *   iou           fp64, the image-level IoU buffer: ovis_coco_box_iou_f64 / ovis_coco_mask_iou_f64 called on `images`.  May
 *                 be NULL when no image has both a detection and a ground truth (nothing reads it).
 *   images        int64 [num_images, 8], the problem-table layout with ONE ROW PER IMAGE: (first detection row, detections,
 *                 first ground-truth row, ground truths, offset of the image's [detections, ground truths] block in `iou`,
 *                 first detection word, first ground-truth word, words per mask).  The last three are not read here.  The
 *                 rows of the images are disjoint; the kernels trust the table (the Python shim checks it on the host).
 *   max_dets, max_gts   the largest detection / ground-truth count of a row of `images`: they size the grids only.
 *   det_category  int32 [num_dets]: the detection's category index.
 *   det_match     int32 [num_dets]: the CHUNK-GLOBAL row of the ground truth the base matched the detection to, or -1.
 *   det_ignore    u8 [num_dets]: the base's ignore flag (a detection matched to a crowd).
 *   gt_category   int32 [num_gts]; gt_crowd u8 [num_gts].
 *   fg_threshold, bg_threshold   t_f and t_b.
 *   err_type      OUT u8 [num_dets]: 0 none (matched or ignored), 1 Cls, 2 Loc, 3 Both, 4 Dupe, 5 Bkg.
 *   err_gt        OUT int32 [num_dets]: the chunk-global row of the target (Cls, Loc, Dupe) or -1.
 *   gt_missed     OUT u8 [num_gts]: 1 for Miss.
 *   Every row an image of the table covers is written.  One wave per detection: lanes stride over the image's ground
 *   truths 64 apart and keep an (IoU, row) maximum for "same" and for "other", two lexicographic butterfly maxima over the
 *   64 lanes follow, lane 0 classifies and stores; a second kernel with one lane per ground truth derives gt_missed from
 *   the finished per-detection arrays.  No atomics, no LDS, no dependence on scheduling: the same bytes on every call.
 *   num_images == 0, or num_dets == 0 and num_gts == 0: OVIS_OK without a launch.  A negative count, or a NULL pointer to
 *   an array whose count is not 0 (images with num_images > 0): OVIS_EINVAL.  More than 2^31 - 1 rows: OVIS_ERANGE.
 *   Python: `_C.error_types(iou, images, det_category, det_match, det_ignore, gt_category, gt_crowd, fg_threshold=0.5,
 *   bg_threshold=0.1) -> (err_type, err_gt, gt_missed)` with `images` a `CocoProblems`. */
int ovis_error_types(const double* iou, const int64_t* images, int num_images, long max_dets, long max_gts,
                     const int32_t* det_category, const int32_t* det_match, const uint8_t* det_ignore,
                     const int32_t* gt_category, const uint8_t* gt_crowd, double fg_threshold, double bg_threshold,
                     long num_dets, long num_gts, uint8_t* err_type, int32_t* err_gt, uint8_t* gt_missed, void* stream);

/* ovis_coco_rle_* / ovis_coco_runs_to_words (csrc/coco_rle_decode.hip): COCO run-length encodings -- the `segmentation` of a
 * results file (what mb/data/datasets/evaluation/coco/coco_eval.py:139-144 writes and COCOeval reads back through
 * pycocotools' rleFrString / rleDecode) or of an RLE annotation -- as the bit words of ovis_coco_pack_masks_u64, for `num`
 * masks of any sizes in one call.  The inverse of ovis_pasted_rle_*; the caller makes the exclusive sums between the stages
 * in the same way.  RLE: column-major runs, zeros first; compressed, value i >= 3 is stored as its difference to value
 * i - 2, in 5-bit groups (low group first, bit 0x20 = "more", the last group's bit 0x10 = the sign), each group + 48.
 *   _count:  chars = all strings of the call concatenated (uint8), char_offsets [num + 1] int64 -> num_runs[p] int32 = the
 *            number of values of string p: its characters c with ((c - 48) & 0x20) == 0.  It only counts.
 *   _runs:   run_offsets [num + 1] int64 with run_offsets[p + 1] - run_offsets[p] >= num_runs[p] -> the decoded values of
 *            string p, differences undone, at runs[run_offsets[p] ..), int32, and status[p] for EVERY p: OVIS_COCO_RLE_OK or
 *            the first of BAD_CHAR (a character outside '0'..'o', 48..111), UNTERMINATED (the last character has the "more"
 *            bit), OVERFLOW (a value of more than 7 characters, or one that does not fit int32 after the sign extension or
 *            after the difference sum).  A string without characters (an uncompressed mask of a mixed call) writes no run
 *            and gets OVIS_COCO_RLE_OK.
 *   ovis_coco_runs_to_words: runs / run_offsets as above -- uncompressed `counts` lists enter here, with status[p] = 0 --
 *            sizes int32 [num, 2] = (height, width), word_offsets [num + 1] int64 (mask p owns ceil(height * width / 64)
 *            words; max_words = the largest such slice, it sizes the grid), run_ends int32 [run_offsets[num]] = scratch (the
 *            inclusive sums of the runs).  status[p] is read and written: a non-zero entry stays; otherwise the first of
 *            BAD_SIZE (height < 1, width < 1 or height * width > 0x7fffffef, the encoder's bound), NEGATIVE_RUN, BAD_SUM
 *            (the runs do not add up to height * width), else OK.  words: pixel p = y * width + x of mask m = bit p % 64
 *            of word p / 64 of its slice, the tail of the last word zero -- ovis_coco_pack_masks_u64's layout, so slices
 *            of both can be concatenated; areas[m] int64 = the sum of the odd-indexed runs.  A mask with non-zero status
 *            gets all-zero words and area 0.  Every word of every slice and every areas / status entry is written.
 * ADDRESSING: every load and store is bounded by char_offsets, run_offsets and word_offsets alone; no decoded value (a
 * character, a run, a sum, a size) is ever an index, a loop bound or a pointer offset.  Arbitrary bytes in chars or runs
 * cannot make a kernel touch memory outside the call's slices -- they only set status.  The offsets themselves are the
 * caller's and are trusted (non-decreasing, inside the buffers).
 * Enqueue only, no atomics, deterministic.  num == 0: OVIS_OK without a launch.  num <= 65535, else OVIS_ERANGE. */
#define OVIS_COCO_RLE_OK 0
#define OVIS_COCO_RLE_BAD_CHAR 1
#define OVIS_COCO_RLE_UNTERMINATED 2
#define OVIS_COCO_RLE_OVERFLOW 3
#define OVIS_COCO_RLE_NEGATIVE_RUN 4
#define OVIS_COCO_RLE_BAD_SUM 5
#define OVIS_COCO_RLE_BAD_SIZE 6
int ovis_coco_rle_count(const uint8_t* chars, const int64_t* char_offsets, int num, int32_t* num_runs, void* stream);
int ovis_coco_rle_runs(const uint8_t* chars, const int64_t* char_offsets, const int64_t* run_offsets, int num,
                       int32_t* runs, int32_t* status, void* stream);
int ovis_coco_runs_to_words(const int32_t* runs, const int64_t* run_offsets, const int32_t* sizes,
                            const int64_t* word_offsets, int num, long max_words, int32_t* run_ends, uint64_t* words,
                            int64_t* areas, int32_t* status, void* stream);

/* ovis_project_rle_masks_f32 (csrc/rle_targets.hip): the mask targets of `num` positives of ONE image straight from the bit
 * words ovis_coco_runs_to_words made of its RLE ground truth -- what the reference computes on a
 * SegmentationMask(mode='mask'): BinaryMaskList.resize (mb/structures/segmentation_mask.py:138-156:
 * F.interpolate(bilinear, align_corners=False), type_as uint8) h0 x w0 -> h1 x w1, .transpose (:113-116: the flips), then
 * project_masks_on_boxes (mb/modeling/roi_heads/mask_head/loss.py:11-42): .crop to the rounded, clamped box
 * (segmentation_mask.py:117-136) and .resize to resolution^2.  A truncated bilinear resample of a 0/1 mask is 1 where the
 * interpolated value reaches 1.0; both resizes are evaluated by the exact form of that: a pixel is 1 iff EVERY tap with a
 * non-zero weight is set (taps and weights: the fp32 expressions of ovis_project_masks_f32).  The reference's fp32 sum
 * departs from it by one rounding on a few per cent of the pixels, in either direction.  No h1 x w1 canvas is written.
 *   words / word_offsets [num_masks + 1]: as ovis_coco_runs_to_words wrote them (absolute offsets into words); every mask
 *   of the image is h0 x w0 and owns words_per_mask = ceil(h0 * w0 / 64) words, else OVIS_ERANGE; pixel (y, x) = bit
 *   (y * w0 + x) % 64 of word (y * w0 + x) / 64 of its slice.  instance [num_instances] int64: the slice of ground truth g;
 *   gt_index [num] int64: the ground truth of positive p; boxes [num, 4] xyxy in the h1 x w1 frame (16-byte aligned);
 *   flip_h / flip_v: the resized mask is mirrored left-right / top-bottom.  out [num, resolution, resolution] f32 in {0, 1}.
 * ADDRESSING: a slice is read only when word_offsets gives it exactly words_per_mask words, at bits below h0 * w0; a
 * gt_index or instance entry outside its count, or such a slice, gives all-zero targets.  No word is used as an address.
 * resolution <= 128, sizes <= 2^24, h0 * w0 <= 0x7fffffef, else OVIS_ERANGE.  One launch, enqueue only, no atomics. */
int ovis_project_rle_masks_f32(const uint64_t* words, const int64_t* word_offsets, int num_masks, long words_per_mask,
                               const int64_t* instance, int num_instances, const int64_t* gt_index, const float* boxes,
                               int num, int h0, int w0, int h1, int w1, int flip_h, int flip_v, int resolution, float* out,
                               void* stream);

/* ovis_project_rle_masks_window_f32: ovis_project_rle_masks_f32 with ONE integer window [win_y, win_y + win_h) x [win_x,
 * win_x + win_w) of the h1 x w1 frame applied behind the flips (BinaryMaskList.crop, segmentation_mask.py:118-136, of the
 * fixed-size crop): decode -> the every-tap rule to h1 x w1 -> flips -> the window -> the box crop on the (win_w, win_h)
 * mask -> the rule again to resolution^2.  boxes are in the WINDOW's frame; a box is rounded and clamped there and the
 * integer offset added afterwards, as cropping a canvas and cropping it again does (rounding box + offset differs when the
 * box lands on a .5 and the offset is odd).  A window that leaves the frame or is empty: OVIS_EINVAL.  With the window
 * equal to the frame the output is bit-equal to ovis_project_rle_masks_f32.  Everything else as there. */
int ovis_project_rle_masks_window_f32(const uint64_t* words, const int64_t* word_offsets, int num_masks, long words_per_mask,
                                      const int64_t* instance, int num_instances, const int64_t* gt_index,
                                      const float* boxes, int num, int h0, int w0, int h1, int w1, int flip_h, int flip_v,
                                      int win_y, int win_x, int win_h, int win_w, int resolution, float* out, void* stream);

/* ovis_proposal_gt_overlaps (csrc/proposal_recall.hip): the matching of the reference's box-proposal recall,
 * evaluate_box_proposals (mb/data/datasets/evaluation/coco/coco_eval.py:199-312; the greedy loop is :269-290, the area
 * test :258, the limit :269-270) over boxlist_iou (mb/structures/boxlist_ops.py:53-89), for a chunk of images, num_areas
 * area ranges and num_limits proposal limits in ONE launch.  images: device int64 [num_images, 4] = (prop_start,
 * prop_count, gt_start, gt_count) over proposals [*, 4] (fp32 xyxy in the ground truth's frame, best objectness first
 * inside an image), gt_boxes [num_gts, 4] (fp32 xyxy) and gt_areas [num_gts] (fp32).  area_ranges [num_areas, 2] fp32,
 * limits [num_limits] int32.  A UNIT is one (image, area range [lo, hi], limit): its ground truths are those with
 * area >= lo && area <= hi, its proposals the first P' = min(prop_count, limit).  min(P', valid ground truths) rounds; each
 * takes the live ground truth whose best IoU over the live proposals is largest (ties: the lowest ground-truth index) and
 * the live proposal that attains it (ties: the lowest proposal index) -- torch.max's first occurrence on both axes --
 * records that IoU for the ground truth and removes both.  A ground truth that overlaps no live proposal still consumes the
 * first live proposal and records 0.
 *   out fp32 [num_areas, num_limits, num_gts]: per ground truth of an image of the table the recorded IoU, 0 when it is
 *   inside the range but was never consumed, -1 when its area is outside the range.  Rows of no image are not written.
 *   IoU: fp32, TO_REMOVE = 1: area = (x2 - x1 + 1) * (y2 - y1 + 1), w = max(min(x2, X2) - max(x1, X1) + 1, 0), h likewise,
 *   iou = w * h / ((area_p + area_g) - w * h), in this operation order without contraction: bit-identical to boxlist_iou.
 *   Boxes must have x2 - x1 + 1 > 0 and y2 - y1 + 1 > 0 (the intersection is then at most either area and the union
 *   positive; a decoded box narrower than a pixel has x2 < x1 by less than 1 and passes); the caller checks.
 * max_gts / max_limit: the largest gt_count of the table / the largest limit; more than OVIS_PROPOSAL_RECALL_MAX_GTS /
 * OVIS_PROPOSAL_RECALL_MAX_LIMIT: OVIS_ERANGE.  The kernel does not check the table against the buffers: the caller does,
 * on the host.  The IoU matrix is never stored; no atomics, no scratch, deterministic and independent of the launch
 * geometry (one workgroup per unit).  num_images == 0: OVIS_OK without a launch.  proposals may be NULL when no image of
 * the table has a proposal. */
#define OVIS_PROPOSAL_RECALL_MAX_GTS 256
#define OVIS_PROPOSAL_RECALL_MAX_LIMIT 1024
int ovis_proposal_gt_overlaps(const float* proposals, const float* gt_boxes, const float* gt_areas, const int64_t* images,
                              int num_images, int max_gts, const float* area_ranges, int num_areas, const int32_t* limits,
                              int num_limits, int max_limit, long num_gts, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OVIS_HIP_H_ */
