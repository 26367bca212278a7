/* C ABI of libovis_cpu.so: the host-side twins of the ops the REFERENCE itself implements on the CPU, for the reference's
 * CPU-only configuration (MODEL.DEVICE=cpu: BASELINE.json configs[0], "plumbing, runs without GPU").
 *
 * The reference dispatches on the tensor's device (maskrcnn_benchmark/csrc/ROIAlign.h:11-25, csrc/nms.h:10-28):
 * device tensors go to the CUDA kernels, host tensors to csrc/cpu/ROIAlign_cpu.cpp:114-219 and csrc/cpu/nms_cpu.cpp:6-65;
 * everything else raises "Not implemented on the CPU" (csrc/ROIAlign.h:44).  `_C.py` keeps exactly that contract: a HOST
 * tensor is served here, a DEVICE tensor only ever by libovis_hip.so -- there is no fallback in either direction, and a
 * missing library raises at the first call that needs it.
 *
 * Plain pointers and sizes, int status (0 = ok, OVIS_CPU_EINVAL = bad argument).  fp32, contiguous NCHW.  `threads` <= 0
 * = all cores (OpenMP); the reference kernels are single-threaded -- the results do not depend on the thread count. */
#ifndef OVIS_CPU_H
#define OVIS_CPU_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define OVIS_CPU_OK 0
#define OVIS_CPU_EINVAL (-1)
#define OVIS_CPU_ERANGE (-3) /* problem size not supported; the value of OVIS_ERANGE (include/ovis_hip.h) */

/* csrc/cpu/ROIAlign_cpu.cpp:114-219 (ROIAlignForward_cpu_kernel): out [R, C, PH, PW]; rois [R, 5] = (batch index, x1, y1, x2, y2)
 * in image pixels; sampling_ratio <= 0 = adaptive ceil(roi extent / bins).  Bit-identical to the reference kernel (same
 * operation order per output, no FMA contraction). */
int ovis_cpu_roi_align_forward_f32(const float* input, const float* rois, float* out, int num_rois, int batch, int channels,
                                   int height, int width, int pooled_h, int pooled_w, float spatial_scale,
                                   int sampling_ratio, int threads);

/* The transpose of the forward (the reference has NO host backward, csrc/ROIAlign.h:44; arithmetic of
 * csrc/cuda/ROIAlign_cuda.cu:178-254 with the atomics replaced by an owner-computes loop: a thread owns whole channel planes
 * and visits the RoIs in order, so the result is deterministic).  grad_input [batch, C, H, W] is overwritten. */
int ovis_cpu_roi_align_backward_f32(const float* grad_out, const float* rois, float* grad_input, int num_rois, int batch,
                                    int channels, int height, int width, int pooled_h, int pooled_w, float spatial_scale,
                                    int sampling_ratio, int threads);

/* csrc/cpu/nms_cpu.cpp:6-65: greedy suppression in descending score order (ties: lower index first), IoU with the "+1"
 * pixel convention, a box is suppressed when IoU >= threshold.  keep [K] receives the ASCENDING original indices of the
 * survivors; returns their number (< 0: bad argument). */
int ovis_cpu_nms_f32(const float* boxes, const float* scores, int num_boxes, float threshold, int64_t* keep);

/* Polygon ground truth -> mask targets: project_masks_on_boxes (mb/modeling/roi_heads/mask_head/loss.py:11-42) for
 * SegmentationMask(mode='poly') -- PolygonInstance.crop / resize / convert_to_binarymask (mb/structures/segmentation_mask.py:270-334,
 * pycocotools==2.0 rleFrPoly + merge + decode).  Host twin of ovis_project_polygon_masks_f32 (include/ovis_hip.h): coords float32
 * (x, y pairs of all polygons), polygon_start int32 [NP + 1] (float offsets), instance_start int32 [G + 1] (polygon ranges),
 * gt_index [num] int64, boxes [num, 4]; out [num, M, M] (1.0 inside). */
int ovis_cpu_project_polygon_masks_f32(const float* coords, const int32_t* polygon_start, const int32_t* instance_start,
                                       const int64_t* gt_index, const float* boxes, int num, int image_width, int image_height,
                                       int resolution, float* out, int threads);

/* Whole-image masks of polygon instances, SegmentationMask(mode='poly').convert('mask') (mb/structures/segmentation_mask.py:326-334:
 * pycocotools frPyObjects -> merge -> decode at the image size).  out [num_instances, height, width] uint8 (1 inside). */
int ovis_cpu_polygons_to_masks_u8(const float* coords, const int32_t* polygon_start, const int32_t* instance_start, int num_instances,
                                  int width, int height, uint8_t* out, int threads);

/* The input transform on host tensors: twin of ovis_transform_images_u8 (include/ovis_hip.h, same layout of `data`, `desc`
 * and `out`, same bits) -- Resize (PIL bilinear, two 8-bit passes), flips, ToTensor, Normalize and to_image_list's zero
 * padding (mb/data/transforms/transforms.py:27-62,65-85,105-120; mb/structures/image_list.py:29-70).  A descriptor that
 * leaves `data` or the canvas: OVIS_CPU_EINVAL.  pad_h, pad_w or an image dimension above 16384, or batch above 65535:
 * OVIS_CPU_ERANGE, as the device entry answers. */
int ovis_cpu_transform_images_u8(const uint8_t* data, long data_bytes, const int32_t* desc, int batch, const float* mean,
                                 const float* std, int to_bgr255, int pad_h, int pad_w, float* out, int threads);

/* The windowed input transform on host tensors (scale jitter + fixed-size crop): twin of ovis_transform_images_window_u8
 * (include/ovis_hip.h states the rule: desc [batch, 11], same layout of `data` and `out`, same bits).  A descriptor that
 * leaves `data`, whose window leaves the resized image or is larger than the canvas: OVIS_CPU_EINVAL.  pad_h, pad_w or an
 * image / resized dimension above 16384, or batch above 65535: OVIS_CPU_ERANGE. */
int ovis_cpu_transform_images_window_u8(const uint8_t* data, long data_bytes, const int32_t* desc, int batch, const float* mean,
                                        const float* std, int to_bgr255, int pad_h, int pad_w, float* out, int threads);

/* Colour jitter on host tensors: twin of ovis_color_jitter_u8 (include/ovis_hip.h states the rule in full: same layout of
 * `data`, `desc`, `ops`, `params` and `out`, same bytes -- PIL's) -- ColorJitter of mb/data/transforms/transforms.py:88-102.
 * A malformed row of `ops` copies its image unchanged, as on the device.  A descriptor that leaves `data`, or `out`
 * overlapping `data`: OVIS_CPU_EINVAL, nothing is written.  An image dimension above 16384 or batch above 65535:
 * OVIS_CPU_ERANGE. */
int ovis_cpu_color_jitter_u8(const uint8_t* data, long data_bytes, const int32_t* desc, const int32_t* ops, const float* params,
                             int batch, uint8_t* out, int threads);

/* The prediction compositor on host tensors: twin of ovis_render_instances_u8 (include/ovis_hip.h: same arguments, same
 * layer kinds, blends and outline rule, same bytes) -- overlay_boxes, overlay_filled_mask and overlay_uncertainty_mask
 * (mb/engine/inference.py:519-589) over the Masker paste (mb/modeling/roi_heads/mask_head/inference.py:124-165).  `boxes`
 * needs no alignment here; every other check answers as the device entry does. */
int ovis_cpu_render_instances_u8(const uint8_t* image, int height, int width, const float* maps, const float* boxes,
                                 int num_layers, int map_resolution, const int32_t* kinds, const float* params,
                                 const float* colors, float alpha, const uint8_t* outline_colors, int outline_thickness,
                                 uint8_t* out, int threads);

/* Box voting and the mean of the views' mask maps on host tensors: twins of ovis_vote_boxes_f32 and
 * ovis_average_view_masks_f32 (include/ovis_hip.h: same arguments, same rule, same float32 operations in the same order --
 * the vote keeps the 64 strided partial sums and the xor butterfly of the device's wavefront, so the bits agree).  Not in
 * the reference (mb/engine/bbox_aug.py:53-69); Detectron's box_voting, scoring method ID.  A kept index outside [0, K), a
 * group outside [0, num_groups) or a kept index outside its group's run: OVIS_CPU_ERANGE, nothing is read through it.
 * `boxes` / `voted` need no alignment here. */
int ovis_cpu_vote_boxes_f32(const float* cand_boxes, const float* cand_scores, const int32_t* offsets,
                            const int32_t* cand_group, long num_candidates, int num_groups, const int64_t* kept,
                            long num_kept, float vote_thresh, float* voted);
int ovis_cpu_average_view_masks_f32(const float* maps, int num_views, long num_maps, int resolution, uint64_t flip_bits,
                                    float* out);

/* Soft-NMS on host tensors: twin of ovis_soft_nms_f32 (include/ovis_hip.h states the rule in full: same arguments, the same
 * float32 operations on the same operands, the Gaussian weight a float64 exponential rounded once -- the same bits), as a
 * plain loop: per round the alive candidate with the largest working score, ties to the lower index, then the decay of the
 * others.  Not in the reference; Bodla et al., ICCV 2017.  `method` takes the values of OVIS_SOFT_NMS_* (0 linear, 1 gaussian,
 * 2 hard).  Malformed offsets (offsets[0] != 0, a negative or decreasing entry, an entry above K, offsets[num_groups] != K):
 * OVIS_CPU_ERANGE, the runs in front of the first such entry are processed and every candidate from there on gets 0.
 * `cand_boxes` needs no alignment here. */
int ovis_cpu_soft_nms_f32(const float* cand_boxes, const float* cand_scores, const int32_t* offsets, long num_candidates,
                          int num_groups, int method, float nms_thresh, float sigma, float min_score, float* soft_scores);

const char* ovis_cpu_version(void);

#ifdef __cplusplus
}
#endif
#endif
