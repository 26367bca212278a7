// Box-proposal recall on the device: the matching of the reference's evaluate_box_proposals
// (data/datasets/evaluation/coco/coco_eval.py:199-312, the loop at :269-290 over boxlist_iou,
// structures/boxlist_ops.py:53-89).  It is NOT COCOeval.evaluateImg (csrc/coco_eval.hip): class-agnostic, one-to-one and
// globally greedy -- every round takes the best-covered ground truth still alive and the live proposal that covers it best,
// records that IoU for the ground truth and removes both.  min(P', G') dependent rounds over a P' x G' fp32 IoU matrix
// that exists nowhere: an entry is recomputed from the two boxes whenever it is needed.
//
//   proposal_recall_kernel   one workgroup per UNIT = (image, area range, limit).  LDS holds the unit's first
//     P' = min(prop_count, limit) proposal boxes, its ground-truth boxes and per ground truth (best IoU over the live
//     proposals, the lowest proposal index that attains it, the recorded result).  A ground truth that is dead -- outside
//     the area range, or consumed -- has best = kDead, so it never wins a round.  The used-proposal set is a bit mask in
//     REGISTERS, one copy per wave: lane l owns proposals l, l + 64, ... (bit s: proposal l + 64 * s; kMaxLimit / 64 = 16
//     bits), and every wave sees every round's winner, so the copies stay equal without any traffic.
//       start   one wave per ground-truth column (wave w: columns w, w + 4, ...), lanes over the proposals, a shuffle
//               butterfly for the lexicographic maximum (IoU descending, proposal index ascending).
//       round   barrier; every wave reduces the columns' (best descending, column ascending) to the same winner (j*, p*)
//               on its own; barrier; thread 0 records best[j*] and kills the column, every wave marks p* used and
//               recomputes those of ITS columns whose argmax was p*.  Nothing else changes: a column's maximum over the
//               live proposals moves only when its argmax leaves.
//     torch.max's first occurrence is the tie rule on both axes (the reference's overlaps.max(dim=0) and
//     max_overlaps.max(dim=0)); used rows and columns are -1 there and every IoU is >= 0, so "first among the live" is the
//     same choice.  The round count min(P', G') (G': the ground truths inside the range, counted once from LDS) is uniform
//     over the workgroup, every loop bound inside a wave is wave-uniform: all barriers and shuffles see whole workgroups /
//     waves.  No atomics, no global scratch; the result does not depend on the launch geometry (one unit, one workgroup).
//   IoU: fp32, TO_REMOVE = 1, boxlist_iou's operation order -- area = (x2 - x1 + 1) * (y2 - y1 + 1),
//     wh = max(min(x2, X2) - max(x1, X1) + 1, 0), iou = inter / ((area1 + area2) - inter); -ffp-contract=off keeps the
//     multiplies and adds apart, the division is hipcc's correctly rounded one.
#include "ovis_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / OVIS_WAVE;
constexpr int kMaxLimit = OVIS_PROPOSAL_RECALL_MAX_LIMIT;  // proposals of a unit: kMaxLimit / 64 bits of the lane's mask
constexpr int kMaxGts = OVIS_PROPOSAL_RECALL_MAX_GTS;
constexpr int kSlots = kMaxLimit / OVIS_WAVE;
constexpr int kNone = 0x7fffffff;
constexpr float kDead = -2.0f;
constexpr int kCols = 4;  // columns of the image table

static_assert(kSlots <= 32, "the used-proposal mask is one 32-bit register per lane");
static_assert(kMaxLimit % OVIS_WAVE == 0 && kMaxGts % OVIS_WAVE == 0, "whole waves");

__device__ __forceinline__ float box_area(const float4 b) { return (b.z - b.x + 1.0f) * (b.w - b.y + 1.0f); }

__device__ __forceinline__ float box_iou(const float4 p, const float p_area, const float4 g, const float g_area) {
  float w = fminf(p.z, g.z) - fmaxf(p.x, g.x) + 1.0f;
  float h = fminf(p.w, g.w) - fmaxf(p.y, g.y) + 1.0f;
  w = w < 0.0f ? 0.0f : w;
  h = h < 0.0f ? 0.0f : h;
  const float inter = w * h;
  return inter / (p_area + g_area - inter);
}

// (IoU descending, index ascending) over the wave: every lane leaves with the same pair
__device__ __forceinline__ void wave_best(float& v, int& idx) {
#pragma unroll
  for (int m = OVIS_WAVE / 2; m >= 1; m >>= 1) {
    const float ov = __shfl_xor(v, m, OVIS_WAVE);
    const int oi = __shfl_xor(idx, m, OVIS_WAVE);
    if (ov > v || (ov == v && oi < idx)) {
      v = ov;
      idx = oi;
    }
  }
}

// column g's maximum over the live proposals, by one whole wave: np and used are the wave's, the result is in every lane
__device__ __forceinline__ void scan_column(const float4* __restrict__ props, int np, unsigned used, int lane, const float4 g,
                                            float& v, int& idx) {
  const float g_area = box_area(g);
  v = -1.0f;
  idx = kNone;
  const int nslots = (np + OVIS_WAVE - 1) / OVIS_WAVE;
  for (int s = 0; s < nslots; ++s) {
    const int p = lane + OVIS_WAVE * s;
    if (p >= np || ((used >> s) & 1u)) continue;
    const float4 b = props[p];
    const float o = box_iou(b, box_area(b), g, g_area);
    if (o > v) {  // p grows with s: an equal IoU stays with the earlier proposal
      v = o;
      idx = p;
    }
  }
  wave_best(v, idx);
}

__global__ __launch_bounds__(kThreads) void proposal_recall_kernel(const float* __restrict__ props,
                                                                   const float* __restrict__ gts,
                                                                   const float* __restrict__ gt_areas,
                                                                   const long long* __restrict__ images,
                                                                   const float* __restrict__ area_ranges, int A,
                                                                   const int* __restrict__ limits, int L, long long G,
                                                                   float* __restrict__ out) {
  __shared__ float4 s_props[kMaxLimit];
  __shared__ float4 s_gts[kMaxGts];
  __shared__ float s_best[kMaxGts];
  __shared__ int s_arg[kMaxGts];
  __shared__ float s_res[kMaxGts];
  const int tid = threadIdx.x, lane = tid & (OVIS_WAVE - 1), wave = tid / OVIS_WAVE;
  const long long unit = blockIdx.x;
  const long long image = unit / ((long long)A * L);
  const int a = (int)((unit / L) % A), l = (int)(unit % L);
  const long long* row = images + kCols * image;
  const long long p0 = row[0], g0 = row[2];
  int np = (int)(row[1] < (long long)kMaxLimit ? row[1] : (long long)kMaxLimit);
  const int limit = limits[l];
  np = np < limit ? np : limit;
  np = np < 0 ? 0 : np;
  // the host entry refuses more than kMaxGts / kMaxLimit; the clamps keep LDS indices in range whatever the table says
  const int ng = (int)(row[3] < (long long)kMaxGts ? row[3] : (long long)kMaxGts);
  const float lo = area_ranges[2 * a], hi = area_ranges[2 * a + 1];

  for (int p = tid; p < np; p += kThreads) {
    const float* b = props + 4 * (p0 + p);
    s_props[p] = make_float4(b[0], b[1], b[2], b[3]);
  }
  for (int j = tid; j < ng; j += kThreads) {
    const float* b = gts + 4 * (g0 + j);
    s_gts[j] = make_float4(b[0], b[1], b[2], b[3]);
    const float ar = gt_areas[g0 + j];
    const bool valid = ar >= lo && ar <= hi;
    s_best[j] = kDead;               // alive only once a proposal has been seen for it
    s_arg[j] = kNone;
    s_res[j] = valid ? 0.0f : -1.0f;
  }
  __syncthreads();

  int num_valid = 0;  // the same in every thread
  for (int j = 0; j < ng; ++j) num_valid += s_res[j] == 0.0f ? 1 : 0;
  const int rounds = np < num_valid ? np : num_valid;
  unsigned used = 0;  // bit s: proposal lane + 64 * s; identical in the four waves' lanes of equal index
  if (rounds > 0) {
    for (int j = wave; j < ng; j += kWaves) {  // j is wave-uniform
      if (s_res[j] != 0.0f) continue;
      float v;
      int idx;
      scan_column(s_props, np, used, lane, s_gts[j], v, idx);
      if (lane == 0 && idx != kNone) {
        s_best[j] = v;
        s_arg[j] = idx;
      }
    }
  }
  const int gslots = (ng + OVIS_WAVE - 1) / OVIS_WAVE;
  for (int r = 0; r < rounds; ++r) {
    __syncthreads();  // the columns the last round (or the start) rewrote are visible
    float v = kDead;
    int jstar = kNone;
    for (int s = 0; s < gslots; ++s) {
      const int j = lane + OVIS_WAVE * s;
      if (j >= ng) continue;
      const float b = s_best[j];
      if (b > v) {  // j grows with s: an equal value stays with the earlier ground truth
        v = b;
        jstar = j;
      }
    }
    wave_best(v, jstar);
    // a live column always has a live proposal while r < min(P', G'); anything else (NaN boxes) ends the unit's rounds here,
    // uniformly: every wave computed the same pair
    const bool none = jstar == kNone || !(v >= 0.0f);
    const int pstar = none ? kNone : s_arg[jstar];
    __syncthreads();  // everyone has read s_best / s_arg of this round
    if (none || pstar < 0 || pstar >= np) break;
    if (tid == 0) {
      s_res[jstar] = v;
      s_best[jstar] = kDead;
    }
    if ((pstar & (OVIS_WAVE - 1)) == lane) used |= 1u << (pstar / OVIS_WAVE);
    if (r + 1 == rounds) break;  // nothing reads the columns again
    for (int j = wave; j < ng; j += kWaves) {
      if (j == jstar) continue;  // thread 0 is writing that one
      if (s_best[j] < 0.0f || s_arg[j] != pstar) continue;
      float nv;
      int idx;
      scan_column(s_props, np, used, lane, s_gts[j], nv, idx);
      if (lane == 0) {
        s_best[j] = idx != kNone ? nv : kDead;
        s_arg[j] = idx;
      }
    }
  }
  __syncthreads();
  float* dst = out + ((long long)a * L + l) * G + g0;
  for (int j = tid; j < ng; j += kThreads) dst[j] = s_res[j];
}

}  // namespace

extern "C" int ovis_proposal_gt_overlaps(const float* proposals, const float* gt_boxes, const float* gt_areas,
                                         const int64_t* images, int num_images, int max_gts, const float* area_ranges,
                                         int num_areas, const int32_t* limits, int num_limits, int max_limit, long num_gts,
                                         float* out, void* stream) {
  if (num_images < 0 || max_gts < 0 || num_areas <= 0 || num_limits <= 0 || max_limit < 0 || num_gts < 0) return OVIS_EINVAL;
  if (num_images == 0) return OVIS_OK;
  if (max_gts > kMaxGts || max_limit > kMaxLimit) return OVIS_ERANGE;
  if (!images || !area_ranges || !limits) return OVIS_EINVAL;
  if (max_gts == 0 || num_gts == 0) return OVIS_OK;  // nothing to write
  if (!gt_boxes || !gt_areas || !out) return OVIS_EINVAL;
  // proposals may be NULL: a table whose images all have prop_count 0 reads none
  const long long units = (long long)num_images * num_areas * num_limits;
  if (units > 0x7fffffffLL) return OVIS_ERANGE;
  hipLaunchKernelGGL(proposal_recall_kernel, dim3((unsigned)units), dim3(kThreads), 0, (hipStream_t)stream, proposals,
                     gt_boxes, gt_areas, (const long long*)images, area_ranges, num_areas, (const int*)limits, num_limits,
                     (long long)num_gts, out);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}
