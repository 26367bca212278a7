// Copy-paste augmentation on the device (include/ovis_hip.h states the rule; it is this project's own, NOT compared with
// any other implementation's output).  Three byte / float movers, all memory bound, no atomics anywhere -- the table and
// every byte are the same on every call:
//   1. paste_alpha_kernel: alpha = OR of the pasted instances' masks, one thread per 16 bytes of alpha.
//   2. own_masks_kernel: ONE workgroup per own mask walks the plane: mask &= ~alpha, the pixel counts before and after and
//      the tight box of what is left; min / max / sum across the lanes of a wave by shuffles, across the waves through LDS.
//   3. paste_images_kernel: in place on the float batch.  One thread owns a pixel position (y, x..x+3) of every channel and
//      EVERY image: it reads the alpha bytes of the images with a source, returns when none is set, else loads the pre-paste
//      values of all images first and stores behind them -- a swap (0 <- 1, 1 <- 0) and a cycle need no second batch.
// A mask plane is h * w bytes at an arbitrary width, so planes are walked as flat byte runs: a scalar head up to the first
// 16-byte boundary of the stream that is STORED (alpha in 1, the own mask in 2), 16-byte chunks, a scalar tail; the stream
// that is only read takes an aligned 16-byte load where its address allows and an unaligned one elsewhere.
#include "ovis_common.h"

namespace {

constexpr int kAlphaThreads = 256;
constexpr int kOwnThreads = 1024;  // 16 waves on one mask plane
constexpr int kOwnWaves = kOwnThreads / OVIS_WAVE;
constexpr int kImageThreads = 256;
constexpr long kMaxPlane = 1L << 30;  // h * w, as ovis_polygons_to_masks_u8

struct alignas(16) Bytes16 {
  unsigned w[4];
};

__device__ __forceinline__ Bytes16 load16(const unsigned char* p) {
  Bytes16 v;
  if (((uintptr_t)p & 15) == 0)
    v = *reinterpret_cast<const Bytes16*>(p);
  else
    __builtin_memcpy(&v, p, 16);
  return v;
}

// 0x01 in every byte of `w` that is not zero
__device__ __forceinline__ unsigned nonzero_bytes(unsigned w) {
  return ((w | ((w & 0x7f7f7f7fu) + 0x7f7f7f7fu)) >> 7) & 0x01010101u;
}

// head / chunks / tail of a run of n bytes whose stored stream starts at address `base`
struct Run {
  long head, chunks, tail;
};
__device__ __forceinline__ Run split_run(const unsigned char* base, long n) {
  Run r;
  r.head = (long)((16 - ((uintptr_t)base & 15)) & 15);
  if (r.head > n) r.head = n;
  r.chunks = (n - r.head) >> 4;
  r.tail = n - r.head - (r.chunks << 4);
  return r;
}

__global__ __launch_bounds__(kAlphaThreads) void paste_alpha_kernel(const unsigned char* __restrict__ paste, int num_paste,
                                                                    long n, unsigned char* __restrict__ alpha) {
  const Run r = split_run(alpha, n);
  const long t = (long)blockIdx.x * kAlphaThreads + threadIdx.x;
  if (t < r.chunks) {
    const long at = r.head + (t << 4);
    Bytes16 acc = {{0u, 0u, 0u, 0u}};
    for (int p = 0; p < num_paste; ++p) {
      const Bytes16 v = load16(paste + (long)p * n + at);
#pragma unroll
      for (int k = 0; k < 4; ++k) acc.w[k] |= v.w[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) acc.w[k] = nonzero_bytes(acc.w[k]);
    *reinterpret_cast<Bytes16*>(alpha + at) = acc;
  }
  if (t < r.head + r.tail) {  // the bytes in front of and behind the chunks
    const long at = t < r.head ? t : r.head + (r.chunks << 4) + (t - r.head);
    unsigned char acc = 0;
    for (int p = 0; p < num_paste; ++p) acc |= paste[(long)p * n + at];
    alpha[at] = acc ? 1 : 0;
  }
}

struct OwnStats {
  int before, after, x1, y1, x2, y2;
};

__device__ __forceinline__ void take_pixel(OwnStats& s, int y, int x) {
  s.x1 = min(s.x1, x);
  s.x2 = max(s.x2, x);
  s.y1 = min(s.y1, y);
  s.y2 = max(s.y2, y);
}

__global__ __launch_bounds__(kOwnThreads) void own_masks_kernel(unsigned char* __restrict__ masks, long n, int width,
                                                                const unsigned char* __restrict__ alpha,
                                                                int* __restrict__ stats) {
  unsigned char* plane = masks + (long)blockIdx.x * n;
  const Run r = split_run(plane, n);
  OwnStats s = {0, 0, 0x7fffffff, 0x7fffffff, -1, -1};
#pragma unroll 2
  for (long c = threadIdx.x; c < r.chunks; c += kOwnThreads) {
    const int at = (int)(r.head + (c << 4));
    Bytes16 m = *reinterpret_cast<const Bytes16*>(plane + at);
    const Bytes16 a = load16(alpha + at);
    unsigned left[4], covered = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned set = nonzero_bytes(m.w[k]), al = nonzero_bytes(a.w[k]);
      left[k] = set & ~al;
      s.before += __popc(set);
      s.after += __popc(left[k]);
      covered |= set & al;
      m.w[k] &= ~(al * 0xffu);
    }
    if (covered) *reinterpret_cast<Bytes16*>(plane + at) = m;  // a chunk alpha leaves as it is needs no store
    if (left[0] | left[1] | left[2] | left[3]) {
      int y = at / width, x = at - y * width;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        if ((left[k >> 2] >> ((k & 3) * 8)) & 1u) take_pixel(s, y, x);
        if (++x == width) {
          x = 0;
          ++y;
        }
      }
    }
  }
  if ((long)threadIdx.x < r.head + r.tail) {
    const int at = (int)(threadIdx.x < r.head ? threadIdx.x : r.head + (r.chunks << 4) + (threadIdx.x - r.head));
    if (plane[at]) {
      ++s.before;
      if (alpha[at]) {
        plane[at] = 0;
      } else {
        ++s.after;
        take_pixel(s, at / width, at % width);
      }
    }
  }
  // across the lanes of a wave, then across the waves through LDS: integer min / max / sum, the same words in any order
#pragma unroll
  for (int d = OVIS_WAVE / 2; d > 0; d >>= 1) {
    s.before += __shfl_xor(s.before, d, OVIS_WAVE);
    s.after += __shfl_xor(s.after, d, OVIS_WAVE);
    s.x1 = min(s.x1, __shfl_xor(s.x1, d, OVIS_WAVE));
    s.y1 = min(s.y1, __shfl_xor(s.y1, d, OVIS_WAVE));
    s.x2 = max(s.x2, __shfl_xor(s.x2, d, OVIS_WAVE));
    s.y2 = max(s.y2, __shfl_xor(s.y2, d, OVIS_WAVE));
  }
  __shared__ OwnStats part[kOwnWaves];
  if ((threadIdx.x & (OVIS_WAVE - 1)) == 0) part[threadIdx.x / OVIS_WAVE] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kOwnWaves; ++w) {
      s.before += part[w].before;
      s.after += part[w].after;
      s.x1 = min(s.x1, part[w].x1);
      s.y1 = min(s.y1, part[w].y1);
      s.x2 = max(s.x2, part[w].x2);
      s.y2 = max(s.y2, part[w].y2);
    }
    int* row = stats + (long)blockIdx.x * 6;
    row[0] = s.before;
    row[1] = s.after;
    row[2] = s.after ? s.x1 : 0;  // an empty remainder: the box (0, 0, -1, -1), which no set pixel can give
    row[3] = s.after ? s.y1 : 0;
    row[4] = s.x2;
    row[5] = s.y2;
  }
}

struct PasteImages {
  const unsigned char* alpha[OVIS_BOX_DECODE_MAX_IMAGES];
  int alpha_h[OVIS_BOX_DECODE_MAX_IMAGES], alpha_w[OVIS_BOX_DECODE_MAX_IMAGES], src[OVIS_BOX_DECODE_MAX_IMAGES];
};

// VEC = 4: pad_w a multiple of 4 and a 16-byte aligned batch, so a thread's four floats are one aligned 16-byte access
template <int VEC>
__global__ __launch_bounds__(kImageThreads) void paste_images_kernel(float* __restrict__ batch, int num_images, int channels,
                                                                     int pad_h, int pad_w, PasteImages im) {
  const int cols = pad_w / VEC;
  const long t = (long)blockIdx.x * kImageThreads + threadIdx.x;
  if (t >= (long)pad_h * cols) return;
  const int y = (int)(t / cols), x = (int)(t - (long)y * cols) * VEC;
  unsigned set[OVIS_BOX_DECODE_MAX_IMAGES];  // per image: bit v = alpha at (y, x + v); outside its frame an alpha is 0
  unsigned any = 0;
#pragma unroll
  for (int i = 0; i < OVIS_BOX_DECODE_MAX_IMAGES; ++i) {
    set[i] = 0;
    if (i < num_images && im.src[i] >= 0 && y < im.alpha_h[i]) {
      const unsigned char* a = im.alpha[i] + (long)y * im.alpha_w[i];
#pragma unroll
      for (int v = 0; v < VEC; ++v)
        if (x + v < im.alpha_w[i] && a[x + v]) set[i] |= 1u << v;
    }
    any |= set[i];
  }
  if (!any) return;
  const long plane = (long)pad_h * pad_w, image = plane * channels;
  for (int c = 0; c < channels; ++c) {
    float* at = batch + c * plane + (long)y * pad_w + x;
    float val[OVIS_BOX_DECODE_MAX_IMAGES][VEC];  // the pre-paste values: every load in front of the first store
#pragma unroll
    for (int i = 0; i < OVIS_BOX_DECODE_MAX_IMAGES; ++i) {
      if (i < num_images && set[i]) {
        const float* from = at + im.src[i] * image;
        if (VEC == 4) {
          const float4 f = *reinterpret_cast<const float4*>(from);
          val[i][0] = f.x, val[i][1] = f.y, val[i][2] = f.z, val[i][3] = f.w;
        } else {
          val[i][0] = from[0];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < OVIS_BOX_DECODE_MAX_IMAGES; ++i) {
      if (i < num_images && set[i]) {
        float* to = at + i * image;
        if (VEC == 4 && set[i] == 0xfu) {
          *reinterpret_cast<float4*>(to) = make_float4(val[i][0], val[i][1], val[i][2], val[i][3]);
        } else {
#pragma unroll
          for (int v = 0; v < VEC; ++v)
            if ((set[i] >> v) & 1u) to[v] = val[i][v];
        }
      }
    }
  }
}

}  // namespace

extern "C" int ovis_copy_paste_masks_u8(uint8_t* masks, int num_own, int num_paste, int height, int width,
                                        uint8_t* alpha_out, int32_t* stats_out, void* stream) {
  if (num_own < 0 || num_paste < 0 || height <= 0 || width <= 0 || !alpha_out) return OVIS_EINVAL;
  if ((num_own + num_paste > 0 && !masks) || (num_own > 0 && !stats_out)) return OVIS_EINVAL;
  const long n = (long)height * width;
  if (n > kMaxPlane) return OVIS_ERANGE;
  const long threads = (n >> 4) + 32;  // at least the chunks, and the at most 30 bytes around them
  hipLaunchKernelGGL(paste_alpha_kernel, dim3((unsigned)ovis_ceil_div(threads, kAlphaThreads)), dim3(kAlphaThreads), 0,
                     (hipStream_t)stream, (const unsigned char*)masks + (long)num_own * n, num_paste, n,
                     (unsigned char*)alpha_out);
  OVIS_LAUNCH_CHECK();
  if (num_own > 0) {
    hipLaunchKernelGGL(own_masks_kernel, dim3((unsigned)num_own), dim3(kOwnThreads), 0, (hipStream_t)stream,
                       (unsigned char*)masks, n, width, (const unsigned char*)alpha_out, (int*)stats_out);
    OVIS_LAUNCH_CHECK();
  }
  return OVIS_OK;
}

extern "C" int ovis_copy_paste_images_f32(float* batch, int num_images, int channels, int pad_h, int pad_w,
                                          const uint8_t* const* alpha_ptrs, const int32_t* alpha_hw,
                                          const int32_t* paste_src, void* stream) {
  if (num_images < 0 || channels <= 0 || pad_h <= 0 || pad_w <= 0) return OVIS_EINVAL;
  if (num_images == 0) return OVIS_OK;
  if (num_images > OVIS_BOX_DECODE_MAX_IMAGES) return OVIS_ERANGE;
  if (!batch || !alpha_ptrs || !alpha_hw || !paste_src) return OVIS_EINVAL;
  if ((long)pad_h * pad_w > kMaxPlane) return OVIS_ERANGE;
  PasteImages im = {};
  bool any = false;
  for (int i = 0; i < num_images; ++i) {
    im.src[i] = paste_src[i];
    if (im.src[i] < -1 || im.src[i] >= num_images) return OVIS_EINVAL;
    if (im.src[i] < 0) continue;
    im.alpha[i] = alpha_ptrs[i];
    im.alpha_h[i] = alpha_hw[2 * i];
    im.alpha_w[i] = alpha_hw[2 * i + 1];
    if (!im.alpha[i] || im.alpha_h[i] <= 0 || im.alpha_w[i] <= 0 || im.alpha_h[i] > pad_h || im.alpha_w[i] > pad_w)
      return OVIS_EINVAL;
    any = true;
  }
  if (!any) return OVIS_OK;
  const bool vec = pad_w % 4 == 0 && ((uintptr_t)batch & 15) == 0;
  const long threads = (long)pad_h * (vec ? pad_w / 4 : pad_w);
  const dim3 grid((unsigned)ovis_ceil_div(threads, kImageThreads));
  if (vec)
    hipLaunchKernelGGL(paste_images_kernel<4>, grid, dim3(kImageThreads), 0, (hipStream_t)stream, batch, num_images, channels,
                       pad_h, pad_w, im);
  else
    hipLaunchKernelGGL(paste_images_kernel<1>, grid, dim3(kImageThreads), 0, (hipStream_t)stream, batch, num_images, channels,
                       pad_h, pad_w, im);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}
