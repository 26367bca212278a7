// COCO scoring on the device: the part of pycocotools' COCOeval (what the reference calls in
// data/datasets/evaluation/coco/coco_eval.py:315-333) whose inputs are image-sized -- the IoU of pasted masks -- and the
// part that has to follow it, COCOeval.evaluateImg's greedy matching.  Accumulate / summarise stay on the host
// (engine/coco_eval.py): they are O(detections) over a few KB per image.
//
// Everything works on a chunk of images at once.  A PROBLEM is one (image, category) pair that has a detection or a
// ground truth; the host lays the chunk's detections out problem after problem (best score first inside a problem, at most
// 100), the ground truths likewise (annotation order inside a problem), and describes the problems in one table
//   int64 [P, 8] = (det_start, det_count, gt_start, gt_count, iou_offset, det_word_start, gt_word_start, words_per_mask)
// iou_offset: where the problem's [det_count, gt_count] fp64 IoU block starts in the chunk's flat IoU buffer; the last
// three (mask IoU only): where the problem's first detection / ground-truth mask starts in the packed-word buffers and
// how many 64-bit words a mask of this image has.  The kernels trust the table: the caller (_C.py) checks every row
// against the buffer sizes on the host before the upload.
//
//   box_iou_kernel    one lane per (detection, ground truth) pair of a problem; fp64, pycocotools' bbIou operation order
//                     (-ffp-contract=off: no FMA), so bit-identical to the formula.
//   pack_masks_kernel [P, HW] bytes -> [P, ceil(HW / 64)] 64-bit words + the pixel count per mask.  A workgroup owns one
//                     mask; a wave reads 8 x 64 consecutive bytes (8 loads in flight per lane), one __ballot per 64 bytes
//                     IS the word (wave64: the ballot is 64 bits wide, lane l -> bit l), lane u keeps word u and the
//                     8 words leave as one 64-byte store.  Bytes past HW read as 0: the tail word is zero-filled.
//   mask_iou_kernel   one wave per pair: popcount of the ANDed words, lanes over words, a shuffle sum; IoU is the ratio
//                     of two integers converted to fp64 -- exact.
//   match_kernel      one wave per (problem, area range, IoU threshold).  Detections are sequential (each one's choice
//                     depends on what the earlier ones took), lanes run over the ground truths: lane l owns ground truths
//                     l, l + 64, ... and keeps their matched / ignored / crowd flags as three 64-bit masks in registers
//                     (so up to 64 * 64 ground truths per problem, more is OVIS_ERANGE), no LDS, no atomics, no barrier.
//                     evaluateImg scans the ground truths sorted non-ignored first and moves to a later one on equal IoU,
//                     stops at the first ignored one once it holds a non-ignored match; that is: among the unmatched
//                     non-ignored ones with iou >= min(t, 1 - 1e-10) the largest IoU, ties to the largest position, else
//                     the same among the ignored ones that are unmatched or crowd.  The stable sort keeps annotation order
//                     inside both groups, so "largest position" is the largest annotation index in the group, and the
//                     choice is ONE lexicographic maximum of (group, iou, index) -- a 6-step shuffle butterfly.
#include "ovis_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / OVIS_WAVE;
constexpr int kPackWords = 8;        // words a wave makes per step
constexpr int kMaxGtSlots = 64;      // ground truths per lane in match_kernel: one bit each of a 64-bit mask
constexpr int kCols = 8;             // columns of the problem table

struct Problem {
  long long d0, nd, g0, ng, off, dw0, gw0, nwords;
};

__device__ __forceinline__ Problem load_problem(const long long* __restrict__ table, long long p) {
  const long long* r = table + kCols * p;
  return Problem{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
}

__global__ __launch_bounds__(kThreads) void box_iou_kernel(const double* __restrict__ dets, const double* __restrict__ gts,
                                                           const unsigned char* __restrict__ crowd,
                                                           const long long* __restrict__ table, double* __restrict__ iou) {
  const Problem pr = load_problem(table, blockIdx.x);
  const long long pairs = pr.nd * pr.ng;
  for (long long k = (long long)blockIdx.y * kThreads + threadIdx.x; k < pairs; k += (long long)gridDim.y * kThreads) {
    const long long i = k / pr.ng, j = k - i * pr.ng;
    const double* d = dets + 4 * (pr.d0 + i);
    const double* g = gts + 4 * (pr.g0 + j);
    const double dx = d[0], dy = d[1], dw = d[2], dh = d[3], gx = g[0], gy = g[1], gw = g[2], gh = g[3];
    double iw = fmin(dx + dw, gx + gw) - fmax(dx, gx);
    double ih = fmin(dy + dh, gy + gh) - fmax(dy, gy);
    iw = iw < 0.0 ? 0.0 : iw;
    ih = ih < 0.0 ? 0.0 : ih;
    const double inter = iw * ih;
    const double uni = crowd[pr.g0 + j] ? dw * dh : dw * dh + gw * gh - inter;
    iou[pr.off + k] = uni == 0.0 ? 0.0 : inter / uni;
  }
}

__global__ __launch_bounds__(kThreads) void pack_masks_kernel(const unsigned char* __restrict__ masks, long long hw,
                                                              long long nwords, unsigned long long* __restrict__ words,
                                                              long long* __restrict__ areas) {
  __shared__ long long partial[kWaves];
  const int lane = threadIdx.x & (OVIS_WAVE - 1), wave = threadIdx.x / OVIS_WAVE;
  const unsigned char* src = masks + (long long)blockIdx.x * hw;
  unsigned long long* dst = words + (long long)blockIdx.x * nwords;
  long long count = 0;  // the same in every lane of the wave
  for (long long w0 = (long long)wave * kPackWords; w0 < nwords; w0 += kWaves * kPackWords) {
    unsigned char v[kPackWords];
#pragma unroll
    for (int u = 0; u < kPackWords; ++u) {
      const long long idx = (w0 + u) * OVIS_WAVE + lane;
      v[u] = idx < hw ? src[idx] : (unsigned char)0;
    }
    unsigned long long mine = 0;
#pragma unroll
    for (int u = 0; u < kPackWords; ++u) {
      const unsigned long long m = __ballot(v[u] != 0);  // all 64 lanes are here: the loop bound is per wave
      count += __popcll(m);
      if (lane == u) mine = m;
    }
    if (lane < kPackWords && w0 + lane < nwords) dst[w0 + lane] = mine;
  }
  if (lane == 0) partial[wave] = count;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long total = 0;
    for (int w = 0; w < kWaves; ++w) total += partial[w];
    areas[blockIdx.x] = total;
  }
}

__global__ __launch_bounds__(kThreads) void mask_iou_kernel(const unsigned long long* __restrict__ dwords,
                                                            const long long* __restrict__ dareas,
                                                            const unsigned long long* __restrict__ gwords,
                                                            const long long* __restrict__ gareas,
                                                            const unsigned char* __restrict__ crowd,
                                                            const long long* __restrict__ table, double* __restrict__ iou) {
  const Problem pr = load_problem(table, blockIdx.x);
  const int lane = threadIdx.x & (OVIS_WAVE - 1), wave = threadIdx.x / OVIS_WAVE;
  const long long pairs = pr.nd * pr.ng;
  for (long long k = (long long)blockIdx.y * kWaves + wave; k < pairs; k += (long long)gridDim.y * kWaves) {  // per wave
    const long long i = k / pr.ng, j = k - i * pr.ng;
    const unsigned long long* a = dwords + pr.dw0 + i * pr.nwords;
    const unsigned long long* b = gwords + pr.gw0 + j * pr.nwords;
    int c = 0;  // <= H * W < 2^31
    for (long long w = lane; w < pr.nwords; w += OVIS_WAVE) c += __popcll(a[w] & b[w]);
#pragma unroll
    for (int m = OVIS_WAVE / 2; m >= 1; m >>= 1) c += __shfl_xor(c, m, OVIS_WAVE);
    if (lane == 0) {
      const long long da = dareas[pr.d0 + i], ga = gareas[pr.g0 + j];
      const long long uni = crowd[pr.g0 + j] ? da : da + ga - c;
      iou[pr.off + k] = uni == 0 ? 0.0 : (double)c / (double)uni;
    }
  }
}

__global__ __launch_bounds__(kThreads) void match_kernel(const double* __restrict__ iou, const long long* __restrict__ table,
                                                         long long num_waves, const double* __restrict__ det_area,
                                                         const double* __restrict__ gt_area,
                                                         const unsigned char* __restrict__ crowd,
                                                         const double* __restrict__ area_rng, int A,
                                                         const double* __restrict__ thrs, int T, long long D, long long G,
                                                         int* __restrict__ dt_match, unsigned char* __restrict__ dt_ignore,
                                                         unsigned char* __restrict__ gt_ignore) {
  const int lane = threadIdx.x & (OVIS_WAVE - 1);
  const long long wid = (long long)blockIdx.x * kWaves + threadIdx.x / OVIS_WAVE;
  if (wid >= num_waves) return;  // whole waves leave: the shuffles below see all 64 lanes
  const long long p = wid / ((long long)A * T);
  const int a = (int)((wid / T) % A), t = (int)(wid % T);
  const Problem pr = load_problem(table, p);
  const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
  const double thr = fmin(thrs[t], 1.0 - 1e-10);
  const int ng = (int)pr.ng;
  int nslots = (ng + OVIS_WAVE - 1) / OVIS_WAVE;
  nslots = nslots > kMaxGtSlots ? kMaxGtSlots : nslots;  // the host entry refuses more; never shift past the mask
  unsigned long long matched = 0, ignored = 0, iscrowd = 0;  // bit s: ground truth lane + 64 * s
  for (int s = 0; s < nslots; ++s) {
    const int j = lane + OVIS_WAVE * s;
    if (j < ng) {
      const bool c = crowd[pr.g0 + j] != 0;
      const double ar = gt_area[pr.g0 + j];
      const bool ig = c || ar < lo || ar > hi;
      ignored |= (unsigned long long)ig << s;
      iscrowd |= (unsigned long long)c << s;
      if (t == 0) gt_ignore[(long long)a * G + pr.g0 + j] = ig;
    }
  }
  for (long long d = 0; d < pr.nd; ++d) {
    int grp = -1, idx = -1;  // group 1: non-ignored, 0: ignored, -1: no candidate
    double best = -1.0;
    const double* row = iou + pr.off + d * pr.ng;
    for (int s = 0; s < nslots; ++s) {
      const int j = lane + OVIS_WAVE * s;
      if (j >= ng) continue;
      if (((matched >> s) & 1) && !((iscrowd >> s) & 1)) continue;
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
      const long long o = ((long long)a * T + t) * D + pr.d0 + d;
      const double ar = det_area[pr.d0 + d];
      dt_match[o] = idx;
      dt_ignore[o] = idx >= 0 ? (unsigned char)(grp == 0) : (unsigned char)(ar < lo || ar > hi);
    }
  }
}

unsigned slices(long max_pairs, int per_block) {
  long s = (max_pairs + per_block - 1) / per_block;
  return (unsigned)(s < 1 ? 1 : (s > 64 ? 64 : s));
}

}  // namespace

extern "C" int ovis_coco_box_iou_f64(const double* dets, const double* gts, const uint8_t* gt_crowd, const int64_t* problems,
                                     int num_problems, long max_pairs, double* iou, void* stream) {
  if (num_problems < 0 || max_pairs < 0) return OVIS_EINVAL;
  if (num_problems == 0 || max_pairs == 0) return OVIS_OK;
  if (!dets || !gts || !gt_crowd || !problems || !iou) return OVIS_EINVAL;
  hipLaunchKernelGGL(box_iou_kernel, dim3((unsigned)num_problems, slices(max_pairs, kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, dets, gts, gt_crowd, (const long long*)problems, iou);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}

extern "C" int ovis_coco_pack_masks_u64(const uint8_t* masks, int num, long pixels, uint64_t* words, int64_t* areas,
                                        void* stream) {
  if (num < 0 || pixels <= 0) return OVIS_EINVAL;
  if (num == 0) return OVIS_OK;
  if (!masks || !words || !areas) return OVIS_EINVAL;
  if (pixels > 0x7fffffffL) return OVIS_ERANGE;  // the intersections are counted in 32 bits
  hipLaunchKernelGGL(pack_masks_kernel, dim3((unsigned)num), dim3(kThreads), 0, (hipStream_t)stream, masks,
                     (long long)pixels, (long long)((pixels + 63) / 64), (unsigned long long*)words, (long long*)areas);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}

extern "C" int ovis_coco_mask_iou_f64(const uint64_t* det_words, const int64_t* det_areas, const uint64_t* gt_words,
                                      const int64_t* gt_areas, const uint8_t* gt_crowd, const int64_t* problems,
                                      int num_problems, long max_pairs, double* iou, void* stream) {
  if (num_problems < 0 || max_pairs < 0) return OVIS_EINVAL;
  if (num_problems == 0 || max_pairs == 0) return OVIS_OK;
  if (!det_words || !det_areas || !gt_words || !gt_areas || !gt_crowd || !problems || !iou) return OVIS_EINVAL;
  hipLaunchKernelGGL(mask_iou_kernel, dim3((unsigned)num_problems, slices(max_pairs, kWaves)), dim3(kThreads), 0,
                     (hipStream_t)stream, (const unsigned long long*)det_words, (const long long*)det_areas,
                     (const unsigned long long*)gt_words, (const long long*)gt_areas, gt_crowd,
                     (const long long*)problems, iou);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}

extern "C" int ovis_coco_match(const double* iou, const int64_t* problems, int num_problems, int max_gts,
                               const double* det_areas, const double* gt_areas, const uint8_t* gt_crowd,
                               const double* area_ranges, int num_areas, const double* thresholds, int num_thresholds,
                               long num_dets, long num_gts, int32_t* dt_match, uint8_t* dt_ignore, uint8_t* gt_ignore,
                               void* stream) {
  if (num_problems < 0 || max_gts < 0 || num_areas <= 0 || num_thresholds <= 0 || num_dets < 0 || num_gts < 0)
    return OVIS_EINVAL;
  if (num_problems == 0) return OVIS_OK;
  if (!problems || !area_ranges || !thresholds) return OVIS_EINVAL;
  if ((num_dets > 0 && (!det_areas || !dt_match || !dt_ignore)) || (num_gts > 0 && (!gt_areas || !gt_crowd || !gt_ignore)))
    return OVIS_EINVAL;
  // iou may be NULL: a table without any (detection, ground truth) pair has an empty IoU buffer, and nothing reads it
  if (max_gts > kMaxGtSlots * OVIS_WAVE) return OVIS_ERANGE;
  const long long waves = (long long)num_problems * num_areas * num_thresholds;
  if ((waves + kWaves - 1) / kWaves > 0x7fffffffLL) return OVIS_ERANGE;
  hipLaunchKernelGGL(match_kernel, dim3((unsigned)((waves + kWaves - 1) / kWaves)), dim3(kThreads), 0, (hipStream_t)stream,
                     iou, (const long long*)problems, waves, det_areas, gt_areas, gt_crowd, area_ranges, num_areas,
                     thresholds, num_thresholds, (long long)num_dets, (long long)num_gts, dt_match, dt_ignore, gt_ignore);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}
