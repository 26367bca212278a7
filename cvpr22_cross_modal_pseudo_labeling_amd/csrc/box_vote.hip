// Box voting and view-averaged masks for test-time augmentation (TEST.BBOX_AUG) on gfx950 (MI355X).
//
// Neither exists in the reference (maskrcnn_benchmark/engine/bbox_aug.py returns the NMS survivors as the views regressed
// them, boxes only).  The voting rule is Detectron's box_voting with scoring method ID: a detection kept by the grouped NMS
// becomes the score-weighted mean of the candidates of its own (image, class) run of the merged list that overlap it by at
// least the vote threshold; scores, labels and order stay.
//
//   box_vote_kernel            one wavefront per kept detection.  Lane l visits candidates lo + l, lo + l + 64, ... of the
//                              run in that order and holds five float32 partials (sum s, sum s*x1, sum s*y1, sum s*x2,
//                              sum s*y2); the 64 partials are reduced by a fixed xor butterfly (32, 16, ... 1), so every
//                              lane ends with the same bits and the result is a pure function of the inputs: no atomics,
//                              no dependence on scheduling.  The IoU is nms.hip's expression operand for operand (this
//                              library is built with -ffp-contract=off), compared with >=: a pair sits on the same side of
//                              a threshold for the NMS and for the vote.
//   average_view_masks_kernel  one thread per output element: ((m_0 + m_1) + m_2) + ... in view order, a mirrored view's
//                              columns reversed, then a DIVISION by float(V) (V == 1 returns its input bit for bit).
//
// Every load of the vote is bounded by `offsets` and K alone: the run [lo, hi) is clamped into [0, K] before it is walked,
// and a kept index outside [0, K), a group outside [0, G) or a kept index outside its group's run writes 1 to *status (a
// plain store of one value, whoever gets there) and zeros to its output row instead of forming an address from it.
#include "ovis_common.h"

namespace {

constexpr int kWave = OVIS_WAVE;
constexpr int kVoteWaves = 4;   // detections per workgroup

// nms.hip::iou_xyxy (devIoU, nms.cu:13-21)
__device__ __forceinline__ float iou_xyxy(const float4 a, const float4 b) {
  const float left = fmaxf(a.x, b.x), right = fminf(a.z, b.z);
  const float top = fmaxf(a.y, b.y), bottom = fminf(a.w, b.w);
  const float width = fmaxf(right - left + 1.f, 0.f), height = fmaxf(bottom - top + 1.f, 0.f);
  const float inter = width * height;
  const float sa = (a.z - a.x + 1.f) * (a.w - a.y + 1.f);
  const float sb = (b.z - b.x + 1.f) * (b.w - b.y + 1.f);
  return inter / (sa + sb - inter);
}

__global__ __launch_bounds__(kVoteWaves * kWave) void box_vote_kernel(
    const float4* __restrict__ cand_boxes, const float* __restrict__ cand_scores, const int* __restrict__ offsets,
    const int* __restrict__ cand_group, long K, int G, const long long* __restrict__ kept, long D, float thr,
    float4* __restrict__ out, int* __restrict__ status) {
  const int lane = threadIdx.x & (kWave - 1);
  const long det = (long)blockIdx.x * kVoteWaves + (threadIdx.x >> 6);   // wave-uniform
  if (det >= D) return;
  const long long d = kept[det];
  bool ok = d >= 0 && d < K;
  long lo = 0, hi = 0;
  if (ok) {
    const int g = cand_group[d];
    ok = g >= 0 && g < G;
    if (ok) {
      lo = offsets[g];
      hi = offsets[g + 1];
      ok = lo >= 0 && hi <= K && d >= lo && d < hi;
    }
  }
  if (!ok) {   // never an address from a bad index
    if (lane == 0) {
      *status = 1;
      out[det] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    return;
  }
  const float4 mine = cand_boxes[d];
  float s = 0.f, x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
  for (long k = lo + lane; k < hi; k += kWave) {
    const float4 b = cand_boxes[k];
    if (iou_xyxy(mine, b) >= thr) {
      const float w = cand_scores[k];
      s = s + w;
      x1 = x1 + w * b.x;
      y1 = y1 + w * b.y;
      x2 = x2 + w * b.z;
      y2 = y2 + w * b.w;
    }
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {   // a + b == b + a bit for bit: all lanes hold the same sums afterwards
    s = s + __shfl_xor(s, off);
    x1 = x1 + __shfl_xor(x1, off);
    y1 = y1 + __shfl_xor(y1, off);
    x2 = x2 + __shfl_xor(x2, off);
    y2 = y2 + __shfl_xor(y2, off);
  }
  if (lane == 0) out[det] = make_float4(x1 / s, y1 / s, x2 / s, y2 / s);
}

__global__ __launch_bounds__(256) void average_view_masks_kernel(const float* __restrict__ maps, int V, long num_maps, int M,
                                                                 unsigned long long flip_bits, float* __restrict__ out) {
  const long per_view = num_maps * M * M;
  const long stride = (long)gridDim.x * blockDim.x;
  const float count = (float)V;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < per_view; i += stride) {
    const int x = (int)(i % M);
    const long mirrored = i - x + (M - 1 - x);
    float acc = maps[(flip_bits & 1ull) ? mirrored : i];
    for (int v = 1; v < V; ++v) acc = acc + maps[(long)v * per_view + (((flip_bits >> v) & 1ull) ? mirrored : i)];
    out[i] = acc / count;
  }
}

}  // namespace

extern "C" int ovis_vote_boxes_f32(const float* cand_boxes, const float* cand_scores, const int32_t* offsets,
                                   const int32_t* cand_group, long num_candidates, int num_groups, const int64_t* kept,
                                   long num_kept, float vote_thresh, float* voted, int32_t* status, void* stream) {
  if (num_candidates < 0 || num_groups < 0 || num_kept < 0) return OVIS_EINVAL;
  if (num_kept == 0) return OVIS_OK;
  if (!kept || !voted || !status || !offsets || ((uintptr_t)voted & 15) != 0) return OVIS_EINVAL;
  if (num_candidates > 0 && (!cand_boxes || !cand_scores || !cand_group || ((uintptr_t)cand_boxes & 15) != 0)) return OVIS_EINVAL;
  if (num_candidates > 2147483647L) return OVIS_ERANGE;   // offsets are int32
  const long blocks = (num_kept + kVoteWaves - 1) / kVoteWaves;
  if (blocks > 2147483647L) return OVIS_ERANGE;
  hipLaunchKernelGGL(box_vote_kernel, dim3((unsigned)blocks), dim3(kVoteWaves * kWave), 0, (hipStream_t)stream,
                     (const float4*)cand_boxes, cand_scores, offsets, cand_group, num_candidates, num_groups,
                     (const long long*)kept, num_kept, vote_thresh, (float4*)voted, status);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}

extern "C" int ovis_average_view_masks_f32(const float* maps, int num_views, long num_maps, int resolution, uint64_t flip_bits,
                                           float* out, void* stream) {
  if (num_views < 1 || num_maps < 0 || resolution < 1) return OVIS_EINVAL;
  if (num_views > 64 || resolution > 32768) return OVIS_ERANGE;   // one flip bit per view
  const long per_view = num_maps * resolution * resolution;
  if ((double)per_view * num_views > 9.0e18) return OVIS_ERANGE;
  if (per_view == 0) return OVIS_OK;
  if (!maps || !out) return OVIS_EINVAL;
  long blocks = (per_view + 255) / 256;
  if (blocks > 16L * OVIS_NUM_CU) blocks = 16L * OVIS_NUM_CU;   // grid-stride beyond that
  hipLaunchKernelGGL(average_view_masks_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, maps, num_views,
                     num_maps, resolution, (unsigned long long)flip_bits, out);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}
