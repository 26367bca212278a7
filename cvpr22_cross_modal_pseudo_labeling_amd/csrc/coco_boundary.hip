// Boundary IoU (Cheng et al., CVPR 2021) on the packed mask words of csrc/coco_eval.hip: the boundary band of a mask and
// the IoU that Boundary AP matches.  The rule is restated in include/ovis_hip.h; in short
//   eroded(m)   = d iterations of a 3x3 erosion with everything outside the image 0
//               = the pixels whose (2d + 1)^2 square lies inside the image and is all set,
//   boundary(m) = m & ~eroded(m),      matched IoU = min(mask IoU, boundary IoU).
//
// A mask is a flat bit stream, pixel p = y * W + x = bit p % 64 of word p / 64; rows are NOT word-aligned.  The square is
// separable, and both halves are windowed ANDs of the flat stream itself:
//   erode_rows_kernel     E[p] = AND_{|k| <= d} m[p + k]      kept where d <= x < W - d   (one column mask per word)
//   erode_columns_kernel  V[p] = AND_{|k| <= d} E[p + k * W]  kept where d <= y < H - d   (one bit range per word)
// No tap needs row handling: where the column condition holds every tap m[p + k] is in row y, where it does not the bit
// is cleared, so bits that reach across a row end never survive; the same for the rows and the image's first / last row.
// A tap is a FUNNEL READ -- 64 bits starting at any bit position, from the two words that hold them; a word outside the
// mask's slice [0, nwords) reads as 0 and is never loaded, so nothing crosses from one mask of the call into the next.
//
// One lane owns one output word (lanes of a wave: consecutive words, so every tap of the wave is two coalesced 512-byte
// reads).  The taps are read straight from global memory: the row pass's 2d + 1 taps come from the same 2 + d / 32 words,
// which are read once and shifted in registers; the column pass's taps lie W bits apart and hit the L1 / L2 -- the
// erode_rows words of a mask are 38 KB at 480 x 640 and 133 KB at 800 x 1333 and are re-read 2d + 1 times by neighbouring
// workgroups of the same mask.  Nothing is staged in LDS, so no size of d * W is special: there is ONE path for every d, H
// and W the entry accepts, and 2d + 1 > 64 is simply a longer loop.  A lane stops at the first tap that leaves it nothing
// (instance masks are mostly empty words: those cost one read); taps go outwards from the centre so that thin structures
// die early.  d is an argument; the host computes max(1, round(0.02 * diagonal)).
//
// Areas: a third launch, one workgroup per mask, popcount + shuffle sum + one LDS word per wave, as pack_masks_kernel.  No
// atomics anywhere, every output word is written by exactly one lane: the same bits on every call.
//
// boundary_iou_kernel is mask_iou_kernel (csrc/coco_eval.hip) over two word buffers per side: both intersections in one
// sweep, both ratios integer / integer in fp64, the smaller one is written.
#include "ovis_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / OVIS_WAVE;
constexpr int kCols = 8;              // columns of the problem table (csrc/coco_eval.hip)
constexpr unsigned kMaxGridY = 65535;

typedef unsigned long long u64;

// bits [lo, hi) of a word, clipped to [0, 64)
__device__ __forceinline__ u64 bit_range(long long lo, long long hi) {
  if (lo < 0) lo = 0;
  if (hi > 64) hi = 64;
  if (lo >= hi) return 0;
  const u64 upto_hi = hi == 64 ? ~0ull : ((1ull << hi) - 1);
  return upto_hi & ~((1ull << lo) - 1);
}

__device__ __forceinline__ u64 word_or_zero(const u64* __restrict__ src, long long nwords, long long q) {
  return (q >= 0 && q < nwords) ? src[q] : 0ull;
}

// the 64 bits of the stream that start at bit position `bit` (any sign); bits outside the slice are 0
__device__ __forceinline__ u64 funnel(const u64* __restrict__ src, long long nwords, long long bit) {
  const long long q = bit >> 6;  // arithmetic shift: floor
  const int r = (int)(bit & 63);
  const u64 lo = word_or_zero(src, nwords, q);
  if (r == 0) return lo;
  const u64 hi = word_or_zero(src, nwords, q + 1);
  return (lo >> r) | (hi << (64 - r));
}

// bit i set: pixel 64 * word + i has d <= x < width - d
__device__ __forceinline__ u64 column_mask(long long word, int width, int d) {
  if (width - d <= d) return 0;
  u64 m = 0;
  long long x = (word * 64) % width;
  for (long long pos = 0; pos < 64; pos += width - x, x = 0)  // pos: the bit where a row's column x sits
    m |= bit_range(pos + d - x, pos + (width - d) - x);
  return m;
}

__global__ __launch_bounds__(kThreads) void erode_rows_kernel(const u64* __restrict__ words, long long nwords, int width,
                                                              int d, long long first_mask, u64* __restrict__ rows) {
  const long long w = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (w >= nwords) return;
  const long long slice = (first_mask + blockIdx.y) * nwords;
  const u64* src = words + slice;
  u64 acc = src[w] & column_mask(w, width, d);
  // taps k = -d .. d start at bit 64 w + k: word q of the stream serves the shifts whose start lies in it
  const long long b0 = w * 64 - d, b1 = w * 64 + d;
  for (long long q = b0 >> 6; acc != 0 && q <= (b1 >> 6); ++q) {
    const u64 lo = word_or_zero(src, nwords, q), hi = word_or_zero(src, nwords, q + 1);
    const int r0 = (int)(b0 > q * 64 ? b0 - q * 64 : 0), r1 = (int)(b1 < q * 64 + 63 ? b1 - q * 64 : 63);
    for (int r = r0; r <= r1; ++r) acc &= r == 0 ? lo : (lo >> r) | (hi << (64 - r));
  }
  rows[slice + w] = acc;
}

__global__ __launch_bounds__(kThreads) void erode_columns_kernel(const u64* __restrict__ words,
                                                                 const u64* __restrict__ rows, long long nwords,
                                                                 int height, int width, int d, long long first_mask,
                                                                 u64* __restrict__ boundary) {
  const long long w = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (w >= nwords) return;
  const long long slice = (first_mask + blockIdx.y) * nwords;
  const u64* src = rows + slice;
  const long long bit = w * 64, pixels = (long long)height * width;
  // d <= y < height - d is one range of the stream
  u64 acc = src[w] & bit_range((long long)d * width - bit, (long long)(height - d) * width - bit);
  for (int k = 1; acc != 0 && k <= d; ++k) {
    acc &= funnel(src, nwords, bit - (long long)k * width);
    acc &= funnel(src, nwords, bit + (long long)k * width);
  }
  boundary[slice + w] = words[slice + w] & ~acc & bit_range(0, pixels - bit);
}

__global__ __launch_bounds__(kThreads) void count_kernel(const u64* __restrict__ words, long long nwords,
                                                         long long first_mask, long long* __restrict__ areas) {
  __shared__ long long partial[kWaves];
  const int lane = threadIdx.x & (OVIS_WAVE - 1), wave = threadIdx.x / OVIS_WAVE;
  const u64* src = words + (first_mask + blockIdx.x) * nwords;
  long long c = 0;
  for (long long w = threadIdx.x; w < nwords; w += kThreads) c += __popcll(src[w]);
#pragma unroll
  for (int m = OVIS_WAVE / 2; m >= 1; m >>= 1) c += __shfl_xor(c, m, OVIS_WAVE);  // every lane is here: no early exit above
  if (lane == 0) partial[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long total = 0;
    for (int v = 0; v < kWaves; ++v) total += partial[v];
    areas[first_mask + blockIdx.x] = total;
  }
}

struct Problem {
  long long d0, nd, g0, ng, off, dw0, gw0, nwords;
};

__device__ __forceinline__ Problem load_problem(const long long* __restrict__ table, long long p) {
  const long long* r = table + kCols * p;
  return Problem{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
}

__device__ __forceinline__ double ratio(long long inter, long long mine, long long other, bool crowd) {
  const long long uni = crowd ? mine : mine + other - inter;
  return uni == 0 ? 0.0 : (double)inter / (double)uni;
}

__global__ __launch_bounds__(kThreads) void boundary_iou_kernel(
    const u64* __restrict__ dwords, const u64* __restrict__ dbwords, const long long* __restrict__ dareas,
    const long long* __restrict__ dbareas, const u64* __restrict__ gwords, const u64* __restrict__ gbwords,
    const long long* __restrict__ gareas, const long long* __restrict__ gbareas, const unsigned char* __restrict__ crowd,
    const long long* __restrict__ table, double* __restrict__ iou) {
  const Problem pr = load_problem(table, blockIdx.x);
  const int lane = threadIdx.x & (OVIS_WAVE - 1), wave = threadIdx.x / OVIS_WAVE;
  const long long pairs = pr.nd * pr.ng;
  for (long long k = (long long)blockIdx.y * kWaves + wave; k < pairs; k += (long long)gridDim.y * kWaves) {  // per wave
    const long long i = k / pr.ng, j = k - i * pr.ng;
    const long long a = pr.dw0 + i * pr.nwords, b = pr.gw0 + j * pr.nwords;
    int c = 0, cb = 0;  // <= H * W < 2^31
    for (long long w = lane; w < pr.nwords; w += OVIS_WAVE) {
      c += __popcll(dwords[a + w] & gwords[b + w]);
      cb += __popcll(dbwords[a + w] & gbwords[b + w]);
    }
#pragma unroll
    for (int m = OVIS_WAVE / 2; m >= 1; m >>= 1) {
      c += __shfl_xor(c, m, OVIS_WAVE);
      cb += __shfl_xor(cb, m, OVIS_WAVE);
    }
    if (lane == 0) {
      const bool cr = crowd[pr.g0 + j] != 0;
      const double mask_iou = ratio(c, dareas[pr.d0 + i], gareas[pr.g0 + j], cr);
      const double bnd_iou = ratio(cb, dbareas[pr.d0 + i], gbareas[pr.g0 + j], cr);
      iou[pr.off + k] = bnd_iou < mask_iou ? bnd_iou : mask_iou;
    }
  }
}

unsigned slices(long max_pairs, int per_block) {
  long s = (max_pairs + per_block - 1) / per_block;
  return (unsigned)(s < 1 ? 1 : (s > 64 ? 64 : s));
}

}  // namespace

extern "C" int ovis_coco_boundary_words_u64(const uint64_t* words, int num, int height, int width, int dilation,
                                            uint64_t* scratch, uint64_t* boundary_words, int64_t* boundary_areas,
                                            void* stream) {
  if (num < 0 || height < 1 || width < 1 || dilation < 1) return OVIS_EINVAL;
  const long long pixels = (long long)height * width;
  if (pixels > 0x7fffffefLL) return OVIS_ERANGE;  // the encoder's pixel bound: every mask word buffer obeys it
  if (num == 0) return OVIS_OK;
  if (!words || !scratch || !boundary_words || !boundary_areas) return OVIS_EINVAL;
  const long long nwords = (pixels + 63) / 64;
  const unsigned blocks = (unsigned)((nwords + kThreads - 1) / kThreads);  // <= 2^25 / 256
  for (long long first = 0; first < num; first += kMaxGridY) {
    const unsigned masks = (unsigned)(num - first < (long long)kMaxGridY ? num - first : (long long)kMaxGridY);
    hipLaunchKernelGGL(erode_rows_kernel, dim3(blocks, masks), dim3(kThreads), 0, (hipStream_t)stream,
                       (const u64*)words, nwords, width, dilation, first, (u64*)scratch);
    OVIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(erode_columns_kernel, dim3(blocks, masks), dim3(kThreads), 0, (hipStream_t)stream,
                       (const u64*)words, (const u64*)scratch, nwords, height, width, dilation, first,
                       (u64*)boundary_words);
    OVIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(count_kernel, dim3(masks), dim3(kThreads), 0, (hipStream_t)stream, (const u64*)boundary_words,
                       nwords, first, (long long*)boundary_areas);
    OVIS_LAUNCH_CHECK();
  }
  return OVIS_OK;
}

extern "C" int ovis_coco_boundary_iou_f64(const uint64_t* det_words, const uint64_t* det_boundary_words,
                                          const int64_t* det_areas, const int64_t* det_boundary_areas,
                                          const uint64_t* gt_words, const uint64_t* gt_boundary_words,
                                          const int64_t* gt_areas, const int64_t* gt_boundary_areas,
                                          const uint8_t* gt_crowd, const int64_t* problems, int num_problems,
                                          long max_pairs, double* iou, void* stream) {
  if (num_problems < 0 || max_pairs < 0) return OVIS_EINVAL;
  if (num_problems == 0 || max_pairs == 0) return OVIS_OK;
  if (!det_words || !det_boundary_words || !det_areas || !det_boundary_areas || !gt_words || !gt_boundary_words ||
      !gt_areas || !gt_boundary_areas || !gt_crowd || !problems || !iou)
    return OVIS_EINVAL;
  hipLaunchKernelGGL(boundary_iou_kernel, dim3((unsigned)num_problems, slices(max_pairs, kWaves)), dim3(kThreads), 0,
                     (hipStream_t)stream, (const u64*)det_words, (const u64*)det_boundary_words,
                     (const long long*)det_areas, (const long long*)det_boundary_areas, (const u64*)gt_words,
                     (const u64*)gt_boundary_words, (const long long*)gt_areas, (const long long*)gt_boundary_areas,
                     gt_crowd, (const long long*)problems, iou);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}
