// Error analysis on the device: the TYPES and MISSED rules of include/ovis_hip.h ("Error analysis") for one chunk of images.
// The base matching (ovis_coco_match at area "all", IoU 0.5) and the IMAGE-LEVEL IoU buffer -- every detection of an image
// against every ground truth of it, other categories included, made by ovis_coco_box_iou_f64 / ovis_coco_mask_iou_f64 on a
// table with one row per image -- come in; nothing image-sized is touched here.
//
//   error_types_kernel  one wave per detection (block x = image, the block's waves stride over its detections).  A matched
//                       or ignored detection is written as (0, -1) by lane 0 and the wave moves on.  For a false positive
//                       the lanes stride over the image's ground truths, 64 apart, reading the detection's contiguous IoU
//                       row; crowds are skipped; each lane keeps an (iou, index) maximum for "same category" and one for
//                       "other category", an equal IoU moving to the later ground truth (the index grows along a lane's
//                       stride).  Two lexicographic (iou, index) butterfly maxima over the 64 lanes follow, and lane 0
//                       classifies with the first rule that holds and stores type and target.  No LDS, no atomics.
//   gt_missed_kernel    one lane per ground truth (block x = image), after error_types_kernel on the same stream: the lane
//                       walks the image's detections and looks for a base match to its row or a Loc / Cls error that
//                       targets it.  Every lane of a wave reads the same detection at the same time: broadcast loads.
// Both kernels write every row their image table covers exactly once from inputs alone: the same bytes on every call.
#include "ovis_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / OVIS_WAVE;
constexpr int kCols = 8;  // columns of the image table: the CocoProblems layout
constexpr unsigned kMaxSlices = 65535;

enum : unsigned char { kNone = 0, kCls = 1, kLoc = 2, kBoth = 3, kDupe = 4, kBkg = 5 };

__device__ __forceinline__ void wave_max(double& v, int& i) {  // the lexicographic maximum of (v, i) in every lane
#pragma unroll
  for (int m = OVIS_WAVE / 2; m >= 1; m >>= 1) {
    const double ov = __shfl_xor(v, m, OVIS_WAVE);
    const int oi = __shfl_xor(i, m, OVIS_WAVE);
    if (ov > v || (ov == v && oi > i)) {
      v = ov;
      i = oi;
    }
  }
}

__global__ __launch_bounds__(kThreads) void error_types_kernel(
    const double* __restrict__ iou, const long long* __restrict__ table, const int* __restrict__ det_cat,
    const int* __restrict__ det_match, const unsigned char* __restrict__ det_ignore, const int* __restrict__ gt_cat,
    const unsigned char* __restrict__ gt_crowd, double t_f, double t_b, unsigned char* __restrict__ err_type,
    int* __restrict__ err_gt) {
  const long long* r = table + kCols * (long long)blockIdx.x;
  const long long d0 = r[0], nd = r[1], g0 = r[2], off = r[4];
  const int ng = (int)r[3];
  const int lane = threadIdx.x & (OVIS_WAVE - 1), wave = threadIdx.x / OVIS_WAVE;
  // wave-uniform bounds: whole waves loop and leave, the shuffles see all 64 lanes
  for (long long d = (long long)blockIdx.y * kWaves + wave; d < nd; d += (long long)gridDim.y * kWaves) {
    const long long row = d0 + d;
    if (det_match[row] >= 0 || det_ignore[row]) {  // wave-uniform
      if (lane == 0) {
        err_type[row] = kNone;
        err_gt[row] = -1;
      }
      continue;
    }
    const int c = det_cat[row];
    const double* v = iou + off + d * ng;
    double s = -1.0, o = -1.0;  // every IoU is >= 0: the first candidate is taken
    int gs = -1, go = -1;
    for (int j = lane; j < ng; j += OVIS_WAVE) {
      if (gt_crowd[g0 + j]) continue;
      const double x = v[j];
      if (gt_cat[g0 + j] == c) {
        if (x >= s) {
          s = x;
          gs = j;
        }
      } else if (x >= o) {
        o = x;
        go = j;
      }
    }
    wave_max(s, gs);
    wave_max(o, go);
    if (lane == 0) {
      if (gs < 0) s = 0.0;  // a maximum over an empty set is 0 with target -1
      if (go < 0) o = 0.0;
      unsigned char type;
      int target = -1;
      if (s >= t_b && s < t_f) {
        type = kLoc;
        target = gs;
      } else if (o >= t_f) {
        type = kCls;
        target = go;
      } else if (s >= t_f) {
        type = kDupe;
        target = gs;
      } else if (fmax(s, o) <= t_b) {
        type = kBkg;
      } else {
        type = kBoth;
      }
      err_type[row] = type;
      err_gt[row] = target < 0 ? -1 : (int)(g0 + target);
    }
  }
}

__global__ __launch_bounds__(kThreads) void gt_missed_kernel(
    const long long* __restrict__ table, const int* __restrict__ det_match, const unsigned char* __restrict__ gt_crowd,
    const unsigned char* __restrict__ err_type, const int* __restrict__ err_gt, unsigned char* __restrict__ gt_missed) {
  const long long* r = table + kCols * (long long)blockIdx.x;
  const long long d0 = r[0], nd = r[1], g0 = r[2], ng = r[3];
  for (long long j = (long long)blockIdx.y * kThreads + threadIdx.x; j < ng; j += (long long)gridDim.y * kThreads) {
    const int g = (int)(g0 + j);
    bool held = gt_crowd[g] != 0;  // a crowd is never missed
    for (long long d = d0; d < d0 + nd && !held; ++d) {
      const unsigned char t = err_type[d];
      held = det_match[d] == g || ((t == kCls || t == kLoc) && err_gt[d] == g);
    }
    gt_missed[g] = held ? 0 : 1;
  }
}

unsigned slices(long n, int per_block) {
  long s = (n + per_block - 1) / per_block;
  s = s < 1 ? 1 : s;
  return (unsigned)(s > (long)kMaxSlices ? (long)kMaxSlices : s);
}

}  // namespace

extern "C" int ovis_error_types(const double* iou, const int64_t* images, int num_images, long max_dets, long max_gts,
                                const int32_t* det_category, const int32_t* det_match, const uint8_t* det_ignore,
                                const int32_t* gt_category, const uint8_t* gt_crowd, double fg_threshold,
                                double bg_threshold, long num_dets, long num_gts, uint8_t* err_type, int32_t* err_gt,
                                uint8_t* gt_missed, void* stream) {
  if (num_images < 0 || max_dets < 0 || max_gts < 0 || num_dets < 0 || num_gts < 0) return OVIS_EINVAL;
  if (num_images == 0 || (num_dets == 0 && num_gts == 0)) return OVIS_OK;
  if (!images) return OVIS_EINVAL;
  if (num_dets > 0 && (!det_category || !det_match || !det_ignore || !err_type || !err_gt)) return OVIS_EINVAL;
  if (num_gts > 0 && (!gt_category || !gt_crowd || !gt_missed)) return OVIS_EINVAL;
  if (num_dets > 0x7fffffffL || num_gts > 0x7fffffffL || max_gts > 0x7fffffffL) return OVIS_ERANGE;  // int32 rows
  // iou may be NULL: a chunk without any (detection, ground truth) pair has an empty IoU buffer, and nothing reads it
  if (num_dets > 0 && max_dets > 0) {
    hipLaunchKernelGGL(error_types_kernel, dim3((unsigned)num_images, slices(max_dets, kWaves)), dim3(kThreads), 0,
                       (hipStream_t)stream, iou, (const long long*)images, det_category, det_match, det_ignore, gt_category,
                       gt_crowd, fg_threshold, bg_threshold, err_type, err_gt);
    OVIS_LAUNCH_CHECK();
  }
  if (num_gts > 0 && max_gts > 0) {
    hipLaunchKernelGGL(gt_missed_kernel, dim3((unsigned)num_images, slices(max_gts, kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, (const long long*)images, det_match, gt_crowd, err_type, err_gt, gt_missed);
    OVIS_LAUNCH_CHECK();
  }
  return OVIS_OK;
}
