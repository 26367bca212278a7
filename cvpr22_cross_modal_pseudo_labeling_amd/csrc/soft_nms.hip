// Soft-NMS (Bodla et al., ICCV 2017: linear, Gaussian; hard for the tie to nms.hip) over the (image, class) runs of a
// candidate list, for gfx950 (MI355X).  The rule is written out in include/ovis_hip.h; nothing like it is in the reference.
//
// The selection order depends on scores that change while the rule runs, so a run is sequential: one ROUND selects the alive
// candidate with the largest working score and decays the others.  Runs are independent: the grid runs over runs.
//
//   ownership   lane l of the T lanes that share a run owns candidates l, l + T, ... of it.  Working scores are read and
//               written by their owner only; a round is one pass of every lane over its own candidates -- decay, discard, and
//               the lane's next local maximum on the way (ascending index and a strict >: the lower index wins a tie) -- and
//               one reduction of the T (score, index) pairs.
//   reduction   in a wavefront a fixed xor butterfly whose compare is "larger score, then lower index": the result does not
//               depend on the lane order.  Across the four wavefronts of a workgroup one LDS slot each, double-buffered by the
//               round's parity, so a round costs ONE barrier (a wave can write round r + 2's slot only behind barrier r + 1,
//               which every wave reaches after it has read round r's).
//   forms       run length <= kWaveCap: one wavefront per run, four runs per workgroup, no barrier (blocks [0, short_blocks));
//               longer: one workgroup per run (blocks [short_blocks, short_blocks + G): block g leaves at once unless run g is
//               long), boxes and working scores in LDS up to kLdsCap candidates, above it the same loop over global memory
//               (boxes from cand_boxes, working scores in soft_scores, negated while alive, so that an entry >= 0 is final).
//               The loop is ONE function over a storage type; every operation of the rule is a separate IEEE operation
//               (-ffp-contract=off), so the forms give the same bits.
//   bounds      a run is touched only after offsets[0 .. g + 1] have been found well-formed (0 first, non-decreasing, <= K):
//               runs in front of the first bad entry are disjoint ranges of [0, K); the wavefront that owns the first bad pair
//               stores 1 to *status and zeros to every candidate from there on; the runs behind it are left alone.  No address
//               is formed from an unchecked value.
#include <climits>

#include "ovis_common.h"

namespace {

constexpr int kWave = OVIS_WAVE;
constexpr int kWaves = 4;                                  // wavefronts per workgroup: runs per workgroup of the one-wave form
constexpr int kThreads = kWaves * kWave;
constexpr int kWaveCap = OVIS_SOFT_NMS_WAVE_CANDIDATES;    // longest run of the one-wave form
constexpr int kLdsCap = OVIS_SOFT_NMS_LDS_CANDIDATES;      // longest run whose boxes and working scores live in LDS

struct Best {
  float w;   // > 0, or 0: nothing alive
  int i;
};

constexpr int kLdsBytes = kLdsCap * (int)(sizeof(float4) + sizeof(float)) + 2 * kWaves * (int)sizeof(Best);
static_assert(kLdsBytes <= 40 * 1024, "four workgroups per CU: a quarter of gfx950's 160 KiB of LDS each (include/ovis_hip.h)");
static_assert(kWaves * kWaveCap <= kLdsCap, "the one-wave form's four runs share the workgroup's arrays");

// nms.hip::iou_xyxy (devIoU, nms.cu:13-21); a = the selected box
__device__ __forceinline__ float iou_xyxy(const float4 a, const float4 b) {
  const float left = fmaxf(a.x, b.x), right = fminf(a.z, b.z);
  const float top = fmaxf(a.y, b.y), bottom = fminf(a.w, b.w);
  const float width = fmaxf(right - left + 1.f, 0.f), height = fmaxf(bottom - top + 1.f, 0.f);
  const float inter = width * height;
  const float sa = (a.z - a.x + 1.f) * (a.w - a.y + 1.f);
  const float sb = (b.z - b.x + 1.f) * (b.w - b.y + 1.f);
  return inter / (sa + sb - inter);
}

__device__ __forceinline__ float decay_weight(int method, float ov, float thr, float sigma) {
  if (method == OVIS_SOFT_NMS_GAUSSIAN) {
    const float q = (ov * ov) / sigma;
    return (float)exp(-(double)q);
  }
  if (!(ov > thr)) return 1.f;
  return method == OVIS_SOFT_NMS_LINEAR ? 1.f - ov : 0.f;
}

// larger score, then lower index: commutative and associative on distinct indices, so any reduction order gives one answer
__device__ __forceinline__ Best better(const Best a, const Best b) {
  return (b.w > a.w || (b.w == a.w && b.i < a.i)) ? b : a;
}

__device__ __forceinline__ Best wave_best(Best v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    Best o;
    o.w = __shfl_xor(v.w, off);
    o.i = __shfl_xor(v.i, off);
    v = better(v, o);
  }
  return v;
}

// The first pair j <= upto of `offsets` that is not well-formed (offsets[0] == 0, 0 <= offsets[j] <= offsets[j + 1] <= K), or
// INT_MAX; the same value in every lane of the calling wavefront.  Reads offsets[0 .. upto + 1], upto < G.
__device__ __forceinline__ int first_bad_pair(const int* __restrict__ offsets, int upto, long K, int lane) {
  int bad = INT_MAX;
  for (int j = lane; j <= upto; j += kWave) {
    const int a = offsets[j], b = offsets[j + 1];
    if ((j == 0 ? a != 0 : a < 0) || a > b || (long)b > K) bad = min(bad, j);
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) bad = min(bad, __shfl_xor(bad, off));
  return bad;
}

// Boxes and working scores of a run in LDS.  score(): > 0 iff alive.
struct LdsRun {
  float4* box;
  float* w;
  float* out;
  __device__ __forceinline__ void load(int k, const float4* __restrict__ boxes) { box[k] = boxes[k]; }
  __device__ __forceinline__ float4 box_of(int k) const { return box[k]; }
  __device__ __forceinline__ float score(int k) const { return w[k]; }
  __device__ __forceinline__ void keep(int k, float v) { w[k] = v; }
  __device__ __forceinline__ void finish(int k, float v) { w[k] = 0.f; out[k] = v; }
};

// The same over global memory: the output holds -w while a candidate is alive (w > 0, a negation is exact), its final value
// (>= 0) afterwards.  An entry is read and written by its owning lane only.
struct GlobalRun {
  const float4* box;
  float* out;
  __device__ __forceinline__ void load(int, const float4* __restrict__) {}
  __device__ __forceinline__ float4 box_of(int k) const { return box[k]; }
  __device__ __forceinline__ float score(int k) const { return -out[k]; }
  __device__ __forceinline__ void keep(int k, float v) { out[k] = -v; }
  __device__ __forceinline__ void finish(int k, float v) { out[k] = v; }
};

// One run of n candidates shared by T lanes (T == kWave: one wavefront, no barrier; T == kThreads: the workgroup, `slots` =
// 2 x kWaves pairs).  boxes / scores point at the run's first candidate.
template <int T, typename Run>
__device__ __forceinline__ void soft_nms_run(Run st, const float4* __restrict__ boxes, const float* __restrict__ scores, int n,
                                             int t, int method, float thr, float sigma, float min_score, Best* slots) {
  Best mine = {0.f, INT_MAX};
  for (int k = t; k < n; k += T) {
    const float s = scores[k];
    st.load(k, boxes);
    if (s > 0.f) {
      st.keep(k, s);
      if (s > mine.w) mine = {s, k};
    } else {
      st.finish(k, 0.f);
    }
  }
  if (T == kWave) {   // the lanes read each other's boxes from LDS: order the wave's stores in front of them
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  int parity = 0;
  for (;;) {
    Best top = wave_best(mine);
    if (T != kWave) {
      Best* slot = slots + parity * kWaves;
      if ((t & (kWave - 1)) == 0) slot[t >> 6] = top;
      __syncthreads();   // the first one also orders the boxes' LDS stores in front of the reads below
      top = slot[0];
#pragma unroll
      for (int v = 1; v < kWaves; ++v) top = better(top, slot[v]);
      parity ^= 1;
    }
    if (!(top.w > 0.f)) break;   // nothing alive: the same decision in every lane
    const float4 sel = st.box_of(top.i);
    if (top.i % T == t) st.finish(top.i, top.w);
    mine = {0.f, INT_MAX};
    for (int k = t; k < n; k += T) {
      float w = st.score(k);
      if (!(w > 0.f)) continue;
      const float ov = iou_xyxy(sel, st.box_of(k));
      w = w * decay_weight(method, ov, thr, sigma);
      if (w >= min_score && w > 0.f) {
        st.keep(k, w);
        if (w > mine.w) mine = {w, k};
      } else {
        st.finish(k, 0.f);
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void soft_nms_kernel(const float4* __restrict__ cand_boxes,
                                                            const float* __restrict__ cand_scores,
                                                            const int* __restrict__ offsets, long K, int G, int short_blocks,
                                                            int method, float thr, float sigma, float min_score,
                                                            float* soft_scores, int* __restrict__ status) {
  __shared__ float4 s_box[kLdsCap];
  __shared__ float s_w[kLdsCap];
  __shared__ Best s_slots[2 * kWaves];
  const int t = threadIdx.x, lane = t & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  if ((int)blockIdx.x < short_blocks) {
    // ---- one wavefront per run; this side also owns the verdict on `offsets` ----
    const int g = (int)blockIdx.x * kWaves + wave;   // wave-uniform
    if (g >= G) return;
    const int bad = first_bad_pair(offsets, g, K, lane);
    if (bad < g) return;   // behind the damage: the owner of pair `bad` has zeroed these candidates
    long zero_from = -1;
    if (bad == g) {
      zero_from = g == 0 ? 0 : (long)offsets[g];   // the end of the well-formed pair g - 1: inside [0, K]
    } else if (g == G - 1 && (long)offsets[G] != K) {
      zero_from = offsets[G];                      // well-formed, so < K: the tail belongs to no run
    }
    if (bad != g) {
      const int lo = offsets[g], n = offsets[g + 1] - lo;
      if (n > 0 && n <= kWaveCap) {
        LdsRun st = {s_box + wave * kWaveCap, s_w + wave * kWaveCap, soft_scores + lo};
        soft_nms_run<kWave>(st, cand_boxes + lo, cand_scores + lo, n, lane, method, thr, sigma, min_score, nullptr);
      }
    }
    if (zero_from >= 0) {
      if (lane == 0) *status = 1;
      for (long k = zero_from + lane; k < K; k += kWave) soft_scores[k] = 0.f;
    }
    return;
  }
  // ---- one workgroup per long run ----
  const int g = (int)blockIdx.x - short_blocks;   // < G by the grid
  const long lo = offsets[g], hi = offsets[g + 1];
  if (lo < 0 || hi > K || hi - lo <= kWaveCap) return;                 // block-uniform
  if (first_bad_pair(offsets, g, K, lane) != INT_MAX) return;         // every wave finds the same answer
  const int n = (int)(hi - lo);
  if (n <= kLdsCap) {
    LdsRun st = {s_box, s_w, soft_scores + lo};
    soft_nms_run<kThreads>(st, cand_boxes + lo, cand_scores + lo, n, t, method, thr, sigma, min_score, s_slots);
  } else {
    GlobalRun st = {cand_boxes + lo, soft_scores + lo};
    soft_nms_run<kThreads>(st, cand_boxes + lo, cand_scores + lo, n, t, method, thr, sigma, min_score, s_slots);
  }
}

}  // namespace

extern "C" int ovis_soft_nms_f32(const float* cand_boxes, const float* cand_scores, const int32_t* offsets, long num_candidates,
                                 int num_groups, int method, float nms_thresh, float sigma, float min_score,
                                 float* soft_scores, int32_t* status, void* stream) {
  if (num_candidates < 0 || num_groups < 0) return OVIS_EINVAL;
  if (method != OVIS_SOFT_NMS_LINEAR && method != OVIS_SOFT_NMS_GAUSSIAN && method != OVIS_SOFT_NMS_HARD) return OVIS_EINVAL;
  if (!(sigma > 0.f) || !(min_score >= 0.f)) return OVIS_EINVAL;
  if (num_candidates == 0 || num_groups == 0) return OVIS_OK;
  if (!cand_boxes || !cand_scores || !offsets || !soft_scores || !status || ((uintptr_t)cand_boxes & 15) != 0) return OVIS_EINVAL;
  if (num_candidates > 2147483647L) return OVIS_ERANGE;   // offsets are int32
  const long short_blocks = ((long)num_groups + kWaves - 1) / kWaves;
  if (short_blocks + num_groups > 2147483647L) return OVIS_ERANGE;
  hipLaunchKernelGGL(soft_nms_kernel, dim3((unsigned)(short_blocks + num_groups)), dim3(kThreads), 0, (hipStream_t)stream,
                     (const float4*)cand_boxes, cand_scores, offsets, num_candidates, num_groups, (int)short_blocks, method,
                     nms_thresh, sigma, min_score, soft_scores, status);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}
