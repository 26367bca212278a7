// Colour jitter on the device (mb/data/transforms/transforms.py:88-102 ColorJitter, first in the training Compose of
// mb/data/transforms/build.py:29-45): the packed RGB uint8 images of ovis_transform_images_u8 -> a second byte buffer of
// the same layout, with the bytes PIL produces (csrc/color_jitter_chain.h, shared with the host twin).  At most two
// launches per batch, whatever B:
//   1. jitter_sum_kernel, only when the caller gave a workspace (some image may hold contrast): per image with contrast, the
//      operations in front of contrast per pixel and the exact integer sum of the grey values -- a wave shuffle reduction,
//      the waves of a block through LDS, one 64-bit integer atomicAdd per block into the image's accumulator (zeroed on the
//      stream).  Integer sums do not depend on the order.
//   2. jitter_apply_kernel: the whole chain for every pixel of every image; an image without operations is copied.
// The stage moves 2 x the raw bytes and nothing else.  Image offsets are multiples of 3, not of 4, so a block owns a run
// of kJitterBlockPixels pixels and moves its 3 * kJitterBlockPixels bytes through an LDS image laid out with the run's
// misalignment: global loads and stores are aligned dwords, consecutive lanes consecutive dwords, with byte accesses only
// for the partial dwords at the two ends of the run; a thread computes kJitterThreadPixels consecutive pixels in place.
#pragma clang fp contract(off)
#include "ovis_common.h"

#define OVIS_HD __host__ __device__ __forceinline__
#include "color_jitter_chain.h"
#include "resample_geom.h"

namespace {

constexpr int kJitterThreads = 256;
constexpr int kJitterThreadPixels = 4;
constexpr int kJitterBlockPixels = kJitterThreads * kJitterThreadPixels;  // 1024 pixels, 3072 bytes
constexpr int kJitterBlockBytes = 3 * kJitterBlockPixels;
constexpr int kJitterSumBlocks = 256;  // per image: the sum kernel strides over an image's runs

struct JitterImage {
  bool valid;
  int offset;
  long pixels;
};

__device__ __forceinline__ JitterImage load_image(const int* __restrict__ desc, int b, long data_bytes, int max_in_h,
                                                  int max_in_w) {
  const int* d = desc + (long)b * kImageDescInts;
  const int offset = d[0], in_h = d[1], in_w = d[2];
  JitterImage im;
  im.valid = jitter_desc_in_buffer(offset, in_h, in_w, data_bytes, max_in_h, max_in_w);
  im.offset = offset;
  im.pixels = im.valid ? (long)in_h * in_w : 0;
  return im;
}

// Bytes [0, nbytes) at `src` -> lds bytes [shift, shift + nbytes), shift = the misalignment the LDS image is laid out with.
// Aligned dwords when src has that misalignment, bytes otherwise and for the partial dwords at the ends; nothing outside
// [src, src + nbytes) is read.
__device__ __forceinline__ void run_to_lds(const unsigned char* __restrict__ src, int nbytes, int shift, unsigned* lds) {
  unsigned char* lb = (unsigned char*)lds;
  const bool aligned = (((uintptr_t)src - (uintptr_t)shift) & 3) == 0;
  const int words = (shift + nbytes + 3) >> 2;
  for (int w = threadIdx.x; w < words; w += kJitterThreads) {
    const int lo = 4 * w - shift;  // of the word's first byte in the run
    if (aligned && lo >= 0 && lo + 4 <= nbytes) {
      lds[w] = *(const unsigned*)(src + lo);
    } else {
      for (int i = 0; i < 4; ++i)
        if (lo + i >= 0 && lo + i < nbytes) lb[4 * w + i] = src[lo + i];
    }
  }
}

__device__ __forceinline__ void lds_to_run(const unsigned* lds, int nbytes, int shift, unsigned char* __restrict__ dst) {
  const unsigned char* lb = (const unsigned char*)lds;
  const int words = (shift + nbytes + 3) >> 2;  // dst has the misalignment `shift`
  for (int w = threadIdx.x; w < words; w += kJitterThreads) {
    const int lo = 4 * w - shift;
    if (lo >= 0 && lo + 4 <= nbytes) {
      *(unsigned*)(dst + lo) = lds[w];
    } else {
      for (int i = 0; i < 4; ++i)
        if (lo + i >= 0 && lo + i < nbytes) dst[lo + i] = lb[4 * w + i];
    }
  }
}

__global__ __launch_bounds__(kJitterThreads) void jitter_sum_kernel(const unsigned char* __restrict__ data, long data_bytes,
                                                                    const int* __restrict__ desc,
                                                                    const int* __restrict__ ops,
                                                                    const float* __restrict__ params, int max_in_h,
                                                                    int max_in_w, unsigned long long* __restrict__ sums) {
  __shared__ unsigned lds[kJitterBlockBytes / 4 + 1];
  __shared__ unsigned long long wave_sum[kJitterThreads / OVIS_WAVE];
  const int b = blockIdx.y;
  const JitterImage im = load_image(desc, b, data_bytes, max_in_h, max_in_w);
  const JitterChain c = jitter_chain(ops + (long)b * kJitterSlots, params + (long)b * kJitterSlots);
  if (!im.valid || c.n < 0 || c.contrast >= c.n) return;  // block-uniform
  const unsigned char* lb = (const unsigned char*)lds;
  unsigned long long sum = 0;
  for (long first = (long)blockIdx.x * kJitterBlockPixels; first < im.pixels; first += (long)gridDim.x * kJitterBlockPixels) {
    const long left = im.pixels - first;
    const int npix = left < kJitterBlockPixels ? (int)left : kJitterBlockPixels;
    const unsigned char* src = data + im.offset + 3 * first;
    const int shift = (int)((uintptr_t)src & 3);
    __syncthreads();  // the previous run has been read
    run_to_lds(src, 3 * npix, shift, lds);
    __syncthreads();
    for (int k = 0; k < kJitterThreadPixels; ++k) {
      const int p = threadIdx.x * kJitterThreadPixels + k;
      if (p < npix) {
        int rgb[3] = {lb[shift + 3 * p], lb[shift + 3 * p + 1], lb[shift + 3 * p + 2]};
        jitter_apply(c, c.contrast, 0, rgb);
        sum += (unsigned)jitter_grey(rgb);
      }
    }
  }
  for (int off = OVIS_WAVE / 2; off > 0; off >>= 1) sum += __shfl_down(sum, off, OVIS_WAVE);
  if ((threadIdx.x & (OVIS_WAVE - 1)) == 0) wave_sum[threadIdx.x / OVIS_WAVE] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kJitterThreads / OVIS_WAVE; ++w) sum += wave_sum[w];
    atomicAdd(sums + b, sum);
  }
}

__global__ __launch_bounds__(kJitterThreads) void jitter_apply_kernel(const unsigned char* __restrict__ data, long data_bytes,
                                                                      const int* __restrict__ desc,
                                                                      const int* __restrict__ ops,
                                                                      const float* __restrict__ params, int max_in_h,
                                                                      int max_in_w,
                                                                      const unsigned long long* __restrict__ sums,
                                                                      unsigned char* __restrict__ out) {
  __shared__ unsigned lds[kJitterBlockBytes / 4 + 1];
  const int b = blockIdx.y;
  const JitterImage im = load_image(desc, b, data_bytes, max_in_h, max_in_w);
  const long first = (long)blockIdx.x * kJitterBlockPixels;
  if (first >= im.pixels) return;  // block-uniform; an invalid descriptor has no pixels: nothing is written
  JitterChain c = jitter_chain(ops + (long)b * kJitterSlots, params + (long)b * kJitterSlots);
  if (c.n < 0 || (c.contrast < c.n && !sums)) c.n = 0;  // malformed, or contrast without its workspace: a copy
  const int mean = c.contrast < c.n ? jitter_contrast_mean((long)sums[b], im.pixels) : 0;
  const long left = im.pixels - first;
  const int npix = left < kJitterBlockPixels ? (int)left : kJitterBlockPixels;
  unsigned char* dst = out + im.offset + 3 * first;
  const int shift = (int)((uintptr_t)dst & 3);  // the LDS image has the misalignment of the stores
  run_to_lds(data + im.offset + 3 * first, 3 * npix, shift, lds);
  __syncthreads();
  if (c.n > 0) {
    unsigned char* lb = (unsigned char*)lds;
    for (int k = 0; k < kJitterThreadPixels; ++k) {
      const int p = threadIdx.x * kJitterThreadPixels + k;
      if (p < npix) {
        unsigned char* px = lb + shift + 3 * p;
        int rgb[3] = {px[0], px[1], px[2]};
        jitter_apply(c, c.n, mean, rgb);
        px[0] = (unsigned char)rgb[0];
        px[1] = (unsigned char)rgb[1];
        px[2] = (unsigned char)rgb[2];
      }
    }
    __syncthreads();
  }
  lds_to_run(lds, 3 * npix, shift, dst);
}

}  // namespace

extern "C" size_t ovis_color_jitter_workspace_bytes(int batch) {
  return batch > 0 ? (size_t)batch * sizeof(unsigned long long) : 0;
}

extern "C" int ovis_color_jitter_u8(const uint8_t* data, long data_bytes, const int32_t* desc, const int32_t* ops,
                                    const float* params, int batch, int max_in_h, int max_in_w, void* workspace,
                                    size_t workspace_bytes, uint8_t* out, void* stream) {
  if (batch < 0 || max_in_h <= 0 || max_in_w <= 0 || data_bytes < 0) return OVIS_EINVAL;
  if (batch == 0) return OVIS_OK;
  if (!data || !desc || !ops || !params || !out) return OVIS_EINVAL;
  if ((uintptr_t)data < (uintptr_t)out + (uintptr_t)data_bytes && (uintptr_t)out < (uintptr_t)data + (uintptr_t)data_bytes)
    return OVIS_EINVAL;  // contrast reads the whole image: no in-place form
  if (max_in_h > kResampleMaxDim || max_in_w > kResampleMaxDim || batch > 65535) return OVIS_ERANGE;
  if (workspace && ((uintptr_t)workspace & 7)) return OVIS_EINVAL;
  if (workspace && workspace_bytes < ovis_color_jitter_workspace_bytes(batch)) return OVIS_ENOSPC;
  const long max_pixels = (long)max_in_h * max_in_w;
  const unsigned runs = (unsigned)ovis_ceil_div(max_pixels, kJitterBlockPixels);
  if (workspace) {
    OVIS_HIP_TRY(hipMemsetAsync(workspace, 0, ovis_color_jitter_workspace_bytes(batch), (hipStream_t)stream));
    hipLaunchKernelGGL(jitter_sum_kernel, dim3(runs < (unsigned)kJitterSumBlocks ? runs : (unsigned)kJitterSumBlocks, (unsigned)batch),
                       dim3(kJitterThreads), 0, (hipStream_t)stream, (const unsigned char*)data, data_bytes, (const int*)desc,
                       (const int*)ops, params, max_in_h, max_in_w, (unsigned long long*)workspace);
    OVIS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(jitter_apply_kernel, dim3(runs, (unsigned)batch), dim3(kJitterThreads), 0, (hipStream_t)stream,
                     (const unsigned char*)data, data_bytes, (const int*)desc, (const int*)ops, params, max_in_h, max_in_w,
                     (const unsigned long long*)workspace, (unsigned char*)out);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}
