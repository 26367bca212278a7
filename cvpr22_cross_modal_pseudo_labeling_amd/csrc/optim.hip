// SGD with momentum and weight decay over MANY tensors in one launch (gfx950).
//
// Reference: maskrcnn_benchmark/solver/build.py:8-37 builds one torch.optim.SGD parameter group per parameter (bias: lr x 2,
// no decay); the update of every parameter is
//     d = g + wd * p;   buf = momentum * buf + d;   p = p - lr * buf            (torch.optim.SGD, dampening 0, no nesterov)
// evaluated by `engine/solver.py::GroupFusedSGD` as six multi-tensor passes (15 tensor reads / writes per element: 2.1 GB
// and 0.44 ms per step for the teacher's 35 M parameters).  Here: one pass -- p, g, buf read, buf, p written (20 bytes per
// element) -- over all tensors that share (lr, wd, momentum), with the SAME fp32 operation sequence and roundings as the
// multi-tensor form (no contraction): bit-identical parameters.
//
// A launch = one group of tensors with common scalars.  `items[i]` = (p, g, buf, n); block b updates elements
// [chunk * kChunk, +kChunk) of item blocks[b].x, chunk = blocks[b].y.  Gradients are views into the reducer's flat buckets
// at arbitrary 4-byte offsets, so the accesses are 4 bytes per lane (a wave still covers 256 contiguous bytes).
#include "ovis_common.h"

namespace {

struct SgdItem {
  float* p;
  const float* g;
  float* buf;  // momentum buffer (ignored when momentum == 0)
  long n;
};

constexpr int kSgdThreads = 256, kSgdChunk = 4096;

__global__ __launch_bounds__(kSgdThreads) void sgd_momentum_multi_kernel(const SgdItem* __restrict__ items,
                                                                        const int2* __restrict__ blocks, float neg_lr,
                                                                        float wd, float momentum, int use_wd) {
  const int2 bc = blocks[blockIdx.x];
  const SgdItem it = items[bc.x];
  const long base = (long)bc.y * kSgdChunk;
  const long end = min(base + kSgdChunk, it.n);
#pragma unroll 4
  for (long i = base + threadIdx.x; i < end; i += kSgdThreads) {
    const float p = it.p[i];
    float d = it.g[i];
    if (use_wd) d = d + p * wd;                 // _foreach_add(grads, _foreach_mul(params, wds))
    float upd = d;
    if (momentum != 0.f) {
      upd = it.buf[i] * momentum + d;           // _foreach_mul_(bufs, momentum); _foreach_add_(bufs, d)
      it.buf[i] = upd;
    }
    it.p[i] = p + upd * neg_lr;                 // _foreach_add_(params, _foreach_mul(upd, -lr))
  }
}

}  // namespace

extern "C" int ovis_sgd_momentum_multi_f32(const void* items, const void* blocks, int num_blocks, float lr,
                                           float weight_decay, float momentum, int apply_weight_decay, void* stream) {
  if (num_blocks < 0) return OVIS_EINVAL;
  if (num_blocks == 0) return OVIS_OK;
  if (!items || !blocks) return OVIS_EINVAL;
  hipLaunchKernelGGL(sgd_momentum_multi_kernel, dim3((unsigned)num_blocks), dim3(kSgdThreads), 0, (hipStream_t)stream,
                     (const SgdItem*)items, (const int2*)blocks, -lr, weight_decay, momentum, apply_weight_decay);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}

extern "C" int ovis_sgd_chunk_elements(void) { return kSgdChunk; }

// ---- SGD + weight EMA in the same pass, and the in-place exchange that puts the averages into the model ------------------
// include/ovis_hip.h states the rule.  The SGD lines are the ones above, in the same order, so p and buf come out with the
// same bits; the average is then moved towards the p that is still in a register:  diff = p_new - e;  e = e + diff * w
// (three roundings, no contraction) -- p, g, buf, e read, buf, p, e written once: 28 bytes per element instead of 20, where
// three multi-tensor passes behind the launch above would move 20 + 32.  Same block table, same 4-byte accesses (the gradient
// views decide the alignment; the kernel is bound by bytes, not by instructions).
namespace {

struct SgdEmaItem {
  float* p;
  const float* g;
  float* buf;  // momentum buffer (ignored when momentum == 0)
  float* ema;
  long n;
};

__global__ __launch_bounds__(kSgdThreads) void sgd_momentum_ema_multi_kernel(const SgdEmaItem* __restrict__ items,
                                                                            const int2* __restrict__ blocks, float neg_lr,
                                                                            float wd, float momentum, int use_wd, float w) {
  const int2 bc = blocks[blockIdx.x];
  const SgdEmaItem it = items[bc.x];
  const long base = (long)bc.y * kSgdChunk;
  const long end = min(base + kSgdChunk, it.n);
#pragma unroll 4
  for (long i = base + threadIdx.x; i < end; i += kSgdThreads) {
    const float p = it.p[i];
    const float e = it.ema[i];
    float d = it.g[i];
    if (use_wd) d = d + p * wd;
    float upd = d;
    if (momentum != 0.f) {
      upd = it.buf[i] * momentum + d;
      it.buf[i] = upd;
    }
    const float pn = p + upd * neg_lr;
    it.p[i] = pn;
    const float diff = pn - e;                  // _foreach_sub(params, emas)
    it.ema[i] = e + diff * w;                   // _foreach_mul_(diff, w); _foreach_add_(emas, diff)
  }
}

struct SwapItem {
  uint32_t* a;
  uint32_t* b;
  long n;
};

// a[i] <-> b[i] as 32-bit words (no float ever holds them: NaN payloads, signed zeros and subnormals pass untouched).
// a and b of an item must not overlap; every word of both is read once and written once by the same lane.
__global__ __launch_bounds__(kSgdThreads) void swap_multi_kernel(const SwapItem* __restrict__ items,
                                                                const int2* __restrict__ blocks) {
  const int2 bc = blocks[blockIdx.x];
  const SwapItem it = items[bc.x];
  const long base = (long)bc.y * kSgdChunk;
  const long end = min(base + kSgdChunk, it.n);
#pragma unroll 4
  for (long i = base + threadIdx.x; i < end; i += kSgdThreads) {
    const uint32_t x = it.a[i], y = it.b[i];
    it.a[i] = y;
    it.b[i] = x;
  }
}

}  // namespace

extern "C" int ovis_sgd_momentum_ema_multi_f32(const void* items, const void* blocks, int num_blocks, float lr,
                                               float weight_decay, float momentum, int apply_weight_decay, float ema_weight,
                                               void* stream) {
  if (num_blocks < 0) return OVIS_EINVAL;
  if (num_blocks == 0) return OVIS_OK;
  if (!items || !blocks) return OVIS_EINVAL;
  hipLaunchKernelGGL(sgd_momentum_ema_multi_kernel, dim3((unsigned)num_blocks), dim3(kSgdThreads), 0, (hipStream_t)stream,
                     (const SgdEmaItem*)items, (const int2*)blocks, -lr, weight_decay, momentum, apply_weight_decay,
                     ema_weight);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}

extern "C" int ovis_swap_multi_f32(const void* items, const void* blocks, int num_blocks, void* stream) {
  if (num_blocks < 0) return OVIS_EINVAL;
  if (num_blocks == 0) return OVIS_OK;
  if (!items || !blocks) return OVIS_EINVAL;
  hipLaunchKernelGGL(swap_multi_kernel, dim3((unsigned)num_blocks), dim3(kSgdThreads), 0, (hipStream_t)stream,
                     (const SwapItem*)items, (const int2*)blocks);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}
