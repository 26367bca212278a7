// LVIS-style federated scoring on the device: the matching of rule 7 / 8 of include/ovis_hip.h ("LVIS-style federated AP").
// Everything image-sized is shared with COCO scoring (csrc/coco_eval.hip, csrc/coco_boundary.hip): the problem table, the flat
// fp64 IoU buffer (non-crowd form: the caller passes all-zero crowd flags to the IoU entries), the packed words.  What differs
// is the matching, and it has an entry and a kernel of its own -- ovis_coco_match is not touched.
//
//   lvis_match_kernel  one wave per (problem, area range, IoU threshold), as match_kernel: detections are sequential, lanes
//                      run over the ground truths (lane l owns l, l + 64, ...; matched / ignored flags are two 64-bit masks
//                      in registers: up to 64 * 64 ground truths, more is OVIS_ERANGE), no LDS, no atomics, no barrier.
//                      Differences to match_kernel: a ground truth's ignore flag is an INPUT flag or the area test (there are
//                      no crowds); a matched ground truth is never a candidate again, ignored or not; an unmatched detection
//                      is ignored when its area is outside the range OR its problem's not-exhaustive flag is set.  The choice
//                      is the same lexicographic maximum of (group, iou, index) by a 6-step shuffle butterfly.
//                      NO-GROUND-TRUTH PATH: most problems of a federated file are a detection or two of a negative category
//                      without any ground truth.  gt_count is wave-uniform, so such a wave takes a branch without divergence:
//                      lanes run over the DETECTIONS, each writes -1 and (area test | problem flag) -- no IoU read, no
//                      shuffle, no sequential loop, coalesced stores.
#include "ovis_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / OVIS_WAVE;
constexpr int kMaxGtSlots = 64;  // ground truths per lane: one bit each of a 64-bit mask
constexpr int kCols = 8;         // columns of the problem table

__global__ __launch_bounds__(kThreads) void lvis_match_kernel(
    const double* __restrict__ iou, const long long* __restrict__ table, long long num_waves,
    const double* __restrict__ det_area, const double* __restrict__ gt_area, const unsigned char* __restrict__ gt_ignore_in,
    const unsigned char* __restrict__ not_exhaustive, const double* __restrict__ area_rng, int A,
    const double* __restrict__ thrs, int T, long long D, long long G, int* __restrict__ dt_match,
    unsigned char* __restrict__ dt_ignore, unsigned char* __restrict__ gt_ignore) {
  const int lane = threadIdx.x & (OVIS_WAVE - 1);
  const long long wid = (long long)blockIdx.x * kWaves + threadIdx.x / OVIS_WAVE;
  if (wid >= num_waves) return;  // whole waves leave: the shuffles below see all 64 lanes
  const long long p = wid / ((long long)A * T);
  const int a = (int)((wid / T) % A), t = (int)(wid % T);
  const long long* r = table + kCols * p;
  const long long d0 = r[0], nd = r[1], g0 = r[2], off = r[4];
  const int ng = (int)r[3];
  const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
  const bool open = not_exhaustive[p] != 0;
  const long long out0 = ((long long)a * T + t) * D + d0;
  if (ng == 0) {  // wave-uniform: nothing to match, every detection is unmatched
    for (long long d = lane; d < nd; d += OVIS_WAVE) {
      const double ar = det_area[d0 + d];
      dt_match[out0 + d] = -1;
      dt_ignore[out0 + d] = (unsigned char)(open || ar < lo || ar > hi);
    }
    return;
  }
  const double thr = fmin(thrs[t], 1.0 - 1e-10);
  int nslots = (ng + OVIS_WAVE - 1) / OVIS_WAVE;
  nslots = nslots > kMaxGtSlots ? kMaxGtSlots : nslots;  // the host entry refuses more; never shift past the mask
  unsigned long long matched = 0, ignored = 0;  // bit s: ground truth lane + 64 * s
  for (int s = 0; s < nslots; ++s) {
    const int j = lane + OVIS_WAVE * s;
    if (j < ng) {
      const double ar = gt_area[g0 + j];
      const bool ig = gt_ignore_in[g0 + j] != 0 || ar < lo || ar > hi;
      ignored |= (unsigned long long)ig << s;
      if (t == 0) gt_ignore[(long long)a * G + g0 + j] = ig;
    }
  }
  for (long long d = 0; d < nd; ++d) {
    int grp = -1, idx = -1;  // group 1: non-ignored, 0: ignored, -1: no candidate
    double best = -1.0;
    const double* row = iou + off + d * ng;
    for (int s = 0; s < nslots; ++s) {
      const int j = lane + OVIS_WAVE * s;
      if (j >= ng) continue;
      if ((matched >> s) & 1) continue;  // never matched again, ignored or not
      const double v = row[j];
      if (v < thr) continue;
      const int g = ((ignored >> s) & 1) ? 0 : 1;
      if (g > grp || (g == grp && v >= best)) {  // j grows with s: an equal IoU moves to the later ground truth
        grp = g;
        best = v;
        idx = j;
      }
    }
#pragma unroll
    for (int m = OVIS_WAVE / 2; m >= 1; m >>= 1) {
      const int og = __shfl_xor(grp, m, OVIS_WAVE), oi = __shfl_xor(idx, m, OVIS_WAVE);
      const double ov = __shfl_xor(best, m, OVIS_WAVE);
      if (og > grp || (og == grp && (ov > best || (ov == best && oi > idx)))) {
        grp = og;
        best = ov;
        idx = oi;
      }
    }
    // every lane now holds the same winner
    if (idx >= 0 && (idx & (OVIS_WAVE - 1)) == lane) matched |= 1ull << (idx / OVIS_WAVE);
    if (lane == 0) {
      const double ar = det_area[d0 + d];
      dt_match[out0 + d] = idx;
      dt_ignore[out0 + d] = idx >= 0 ? (unsigned char)(grp == 0) : (unsigned char)(open || ar < lo || ar > hi);
    }
  }
}

}  // namespace

extern "C" int ovis_lvis_match(const double* iou, const int64_t* problems, int num_problems, int max_gts,
                               const double* det_areas, const double* gt_areas, const uint8_t* gt_ignore_in,
                               const uint8_t* problem_not_exhaustive, const double* area_ranges, int num_areas,
                               const double* thresholds, int num_thresholds, long num_dets, long num_gts, int32_t* dt_match,
                               uint8_t* dt_ignore, uint8_t* gt_ignore, void* stream) {
  if (num_problems < 0 || max_gts < 0 || num_areas <= 0 || num_thresholds <= 0 || num_dets < 0 || num_gts < 0)
    return OVIS_EINVAL;
  if (num_problems == 0) return OVIS_OK;
  if (!problems || !problem_not_exhaustive || !area_ranges || !thresholds) return OVIS_EINVAL;
  if ((num_dets > 0 && (!det_areas || !dt_match || !dt_ignore)) ||
      (num_gts > 0 && (!gt_areas || !gt_ignore_in || !gt_ignore)))
    return OVIS_EINVAL;
  // iou may be NULL: a table without any (detection, ground truth) pair has an empty IoU buffer, and nothing reads it
  if (max_gts > kMaxGtSlots * OVIS_WAVE) return OVIS_ERANGE;
  const long long waves = (long long)num_problems * num_areas * num_thresholds;
  if ((waves + kWaves - 1) / kWaves > 0x7fffffffLL) return OVIS_ERANGE;
  hipLaunchKernelGGL(lvis_match_kernel, dim3((unsigned)((waves + kWaves - 1) / kWaves)), dim3(kThreads), 0,
                     (hipStream_t)stream, iou, (const long long*)problems, waves, det_areas, gt_areas, gt_ignore_in,
                     problem_not_exhaustive, area_ranges, num_areas, thresholds, num_thresholds, (long long)num_dets,
                     (long long)num_gts, dt_match, dt_ignore, gt_ignore);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}
