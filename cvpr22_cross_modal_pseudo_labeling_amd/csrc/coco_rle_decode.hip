// COCO run-length encodings back to the scorer's bit words: the inverse of csrc/mask_rle.hip, for the masks of a results
// file (segm.json) and RLE ground truth.  pycocotools' rleFrString (common/maskApi.c) + rleDecode, restated, with the
// transpose from the RLE's column-major order to ovis_coco_pack_masks_u64's row-major bit order folded in -- no byte mask is
// ever written.  Three stages, as the encoder's (the caller makes the exclusive sums between them):
//
//   coco_rle_count_kernel   one workgroup per string: the number of values = the characters c with ((c - 48) & 0x20) == 0
//   coco_rle_runs_kernel    one workgroup per string, 256 characters a round.  The lane that holds a value's LAST character
//                           assembles it from the (at most 7) characters in front of it in LDS, most significant group
//                           first; its index is a scan over the terminators; the difference coding
//                           (counts[i] += counts[i - 2], i >= 3) is two more scans, over the even (2, 4, ...) and the odd
//                           (1, 3, ...) indices, carried from round to round in int64
//   coco_run_ends_kernel    one workgroup per mask: validates size and runs, writes the inclusive sums of the runs (the
//                           pixel behind every run, in column-major order) and the area = the sum of the odd-indexed runs
//   coco_words_kernel       one wavefront per output word: lane l holds row-major pixel p = 64 * word + l = (y, x), finds
//                           the run that holds q = x * H + y by binary search in the mask's run ends, and the word is the
//                           __ballot of the run index's parity
//
// ADDRESSING.  Every load and store is bounded by char_offsets, run_offsets and word_offsets alone.  A decoded value -- a
// character, a run, a run end -- is compared, added and stored, but never used as an index, a loop bound or a pointer
// offset: the searches move inside [0, slots of this mask), the loops run over slices.  Arbitrary bytes in `chars` or
// `runs` therefore cannot make a kernel touch memory outside its slices; they can only set `status`.  The image size
// decides which pixel a lane stands for, never where it loads or stores.
//
// The run ends live in global memory and are searched there: a mask's ends (a few hundred int32 for a detection, a few
// thousand for noise) are read by every wavefront of that mask, so they stay in the vector L1 / L2 of the CUs that work
// on it; staging them in LDS would cost every 4-word workgroup a full copy.  No atomics; the same words on every call.
#include "ovis_common.h"

namespace {

constexpr int kDecThreads = 256;
constexpr int kDecWaves = kDecThreads / OVIS_WAVE;
constexpr int kDecHalo = 7;                   // the characters in front of a terminator that can belong to its value
constexpr long kDecMaxPixels = 0x7fffffefL;   // the encoder's bound (csrc/mask_rle.hip): x * H + y fits a signed 32-bit word
constexpr long kInt32Min = -2147483648L, kInt32Max = 2147483647L;

constexpr int kFlagChar = 1, kFlagOpen = 2, kFlagOverflow = 4;

// a value ends at a character for which this is false
__device__ __forceinline__ bool continues(unsigned char c) { return (((int)c - 48) & 0x20) != 0; }

// inclusive prefix of v over the workgroup's lanes in thread order; *total = the sum.  Ends with a barrier in front of which
// every lane has read wave_total, so the caller may use it again at once.
__device__ __forceinline__ long block_inclusive_scan(long v, long* wave_total, long* total) {
  const int lane = threadIdx.x & (OVIS_WAVE - 1), wave = threadIdx.x / OVIS_WAVE;
  long incl = v;
#pragma unroll
  for (int off = 1; off < OVIS_WAVE; off <<= 1) {
    const long up = __shfl_up(incl, off);
    if (lane >= off) incl += up;
  }
  if (lane == OVIS_WAVE - 1) wave_total[wave] = incl;
  __syncthreads();
  long before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < kDecWaves; ++k) {
    const long s = wave_total[k];
    before += k < wave ? s : 0;
    all += s;
  }
  __syncthreads();
  *total = all;
  return before + incl;
}

// the OR of v over the workgroup, in every lane
__device__ __forceinline__ int block_or(int v, int* wave_bits) {
#pragma unroll
  for (int off = OVIS_WAVE / 2; off > 0; off >>= 1) v |= __shfl_xor(v, off);
  if ((threadIdx.x & (OVIS_WAVE - 1)) == 0) wave_bits[threadIdx.x / OVIS_WAVE] = v;
  __syncthreads();
  int all = 0;
#pragma unroll
  for (int k = 0; k < kDecWaves; ++k) all |= wave_bits[k];
  __syncthreads();
  return all;
}

__global__ __launch_bounds__(kDecThreads) void coco_rle_count_kernel(const unsigned char* __restrict__ chars,
                                                                    const long* __restrict__ char_offsets,
                                                                    int* __restrict__ num_runs) {
  __shared__ long wave_total[kDecWaves];
  const int p = blockIdx.x;
  const long begin = char_offsets[p], end = char_offsets[p + 1];
  long mine = 0;
  for (long i = begin + threadIdx.x; i < end; i += kDecThreads) mine += continues(chars[i]) ? 0 : 1;
  long total;
  block_inclusive_scan(mine, wave_total, &total);
  if (threadIdx.x == 0) num_runs[p] = (int)(total > kInt32Max ? kInt32Max : total);
}

__global__ __launch_bounds__(kDecThreads) void coco_rle_runs_kernel(const unsigned char* __restrict__ chars,
                                                                   const long* __restrict__ char_offsets,
                                                                   const long* __restrict__ run_offsets,
                                                                   int* __restrict__ runs_all, int* __restrict__ status) {
  __shared__ long wave_total[kDecWaves];
  __shared__ int wave_bits[kDecWaves];
  __shared__ unsigned char text[kDecHalo + kDecThreads];
  const int p = blockIdx.x, tid = threadIdx.x;
  const long begin = char_offsets[p], end = char_offsets[p + 1];
  const long slots = run_offsets[p + 1] - run_offsets[p];  // the values this string may write
  int* runs = runs_all + run_offsets[p];
  int flags = 0;
  long index_carry = 0, sum_carry[2] = {0, 0};  // values so far; the running sums of the even and the odd chain
  for (long base = begin; base < end; base += kDecThreads) {  // workgroup-uniform
    const long i = base + tid;
    const bool has = i < end;
    // the round's characters behind a halo of the kDecHalo in front of them; '0' (a terminator) in front of the string
    text[kDecHalo + tid] = has ? chars[i] : (unsigned char)48;
    if (tid < kDecHalo) text[tid] = base - kDecHalo + tid >= begin ? chars[base - kDecHalo + tid] : (unsigned char)48;
    __syncthreads();
    const unsigned char c = text[kDecHalo + tid];
    const bool last = has && !continues(c);
    if (has && (c < 48 || c > 111)) flags |= kFlagChar;
    if (has && i == end - 1 && !last) flags |= kFlagOpen;
    long x = 0;
    if (last) {
      const int g = ((int)c - 48) & 0x1f;
      x = (g & 0x10) ? g - 32 : g;  // the top group carries the sign
      bool open = true;
#pragma unroll
      for (int j = 1; j <= kDecHalo; ++j) {  // a fixed walk over the halo; `open` goes out at the value in front
        const unsigned char b = text[kDecHalo + tid - j];
        open = open && continues(b);
        if (open && j < kDecHalo) x = x * 32 + (((int)b - 48) & 0x1f);
        if (open && j == kDecHalo) flags |= kFlagOverflow;  // an eighth character: more than 35 bits
      }
      if (x < kInt32Min || x > kInt32Max) flags |= kFlagOverflow;
    }
    long round_values;
    const long index = index_carry + block_inclusive_scan(last ? 1 : 0, wave_total, &round_values) - 1;  // of this value
    // counts[i] += counts[i - 2] for i >= 3: index 0 stands alone, 2, 4, ... and 1, 3, ... are running sums
    long value = x;
#pragma unroll
    for (int parity = 0; parity < 2; ++parity) {
      const bool in_chain = last && index > 0 && (index & 1) == parity;
      long round_sum;
      const long incl = sum_carry[parity] + block_inclusive_scan(in_chain ? x : 0, wave_total, &round_sum);
      if (in_chain) value = incl;
      sum_carry[parity] += round_sum;
    }
    if (last) {
      if (value < kInt32Min || value > kInt32Max) flags |= kFlagOverflow;
      if (index < slots) runs[index] = (int)value;  // beyond cannot happen with the count of the same string
    }
    index_carry += round_values;
  }
  flags = block_or(flags, wave_bits);
  if (tid == 0)
    status[p] = (flags & kFlagChar) ? OVIS_COCO_RLE_BAD_CHAR
                : (flags & kFlagOpen) ? OVIS_COCO_RLE_UNTERMINATED
                : (flags & kFlagOverflow) ? OVIS_COCO_RLE_OVERFLOW : OVIS_COCO_RLE_OK;
}

__global__ __launch_bounds__(kDecThreads) void coco_run_ends_kernel(const int* __restrict__ runs_all,
                                                                   const long* __restrict__ run_offsets,
                                                                   const int* __restrict__ sizes, int* __restrict__ ends_all,
                                                                   long* __restrict__ areas, int* __restrict__ status) {
  __shared__ long wave_total[kDecWaves];
  __shared__ int wave_bits[kDecWaves];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int entry = status[p];  // what ovis_coco_rle_runs found, or the caller's 0
  if (entry != OVIS_COCO_RLE_OK) {  // workgroup-uniform
    if (tid == 0) areas[p] = 0;
    return;
  }
  const long n = run_offsets[p + 1] - run_offsets[p];
  const int* runs = runs_all + run_offsets[p];
  int* ends = ends_all + run_offsets[p];
  const long H = sizes[2 * p], W = sizes[2 * p + 1];
  long carry = 0, odd = 0;
  int negative = 0;
  for (long base = 0; base < n; base += kDecThreads) {  // workgroup-uniform
    const long k = base + tid;
    const long r = k < n ? runs[k] : 0;
    negative |= r < 0 ? 1 : 0;
    odd += (k & 1) ? r : 0;
    long round_total;
    const long incl = carry + block_inclusive_scan(r, wave_total, &round_total);
    // a good mask's sums are at most H * W <= kDecMaxPixels; a bad one's are never read
    if (k < n) ends[k] = (int)(incl < 0 ? 0 : incl > kInt32Max ? kInt32Max : incl);
    carry += round_total;
  }
  long area;
  block_inclusive_scan(odd, wave_total, &area);
  negative = block_or(negative, wave_bits);
  if (tid == 0) {
    const int verdict = (H < 1 || W < 1 || H * W > kDecMaxPixels) ? OVIS_COCO_RLE_BAD_SIZE
                        : negative ? OVIS_COCO_RLE_NEGATIVE_RUN
                        : carry != H * W ? OVIS_COCO_RLE_BAD_SUM : OVIS_COCO_RLE_OK;
    status[p] = verdict;
    areas[p] = verdict == OVIS_COCO_RLE_OK ? area : 0;
  }
}

__global__ __launch_bounds__(kDecThreads) void coco_words_kernel(const int* __restrict__ ends_all,
                                                                const long* __restrict__ run_offsets,
                                                                const int* __restrict__ sizes,
                                                                const long* __restrict__ word_offsets,
                                                                const int* __restrict__ status,
                                                                unsigned long long* __restrict__ words_all) {
  const int m = blockIdx.y, lane = threadIdx.x & (OVIS_WAVE - 1);
  const long word = (long)blockIdx.x * kDecWaves + threadIdx.x / OVIS_WAVE;  // wavefront-uniform
  const long num_words = word_offsets[m + 1] - word_offsets[m];
  if (word >= num_words) return;
  const long n = run_offsets[m + 1] - run_offsets[m];
  const int* ends = ends_all + run_offsets[m];
  const long H = sizes[2 * m], W = sizes[2 * m + 1];
  const bool good = status[m] == OVIS_COCO_RLE_OK && n >= 1;  // then H, W >= 1 and ends[n - 1] = H * W
  const long pixel = word * 64 + lane;
  bool bit = false;
  if (good && pixel < H * W) {
    const unsigned y = (unsigned)pixel / (unsigned)W, x = (unsigned)pixel - y * (unsigned)W;  // H * W fits 31 bits
    const long q = (long)x * H + y;  // < H * W = ends[n - 1]
    long lo = 0, hi = n - 1;   // the first run whose end is behind q: positions inside [0, n - 1] whatever the ends hold
    while (lo < hi) {
      const long mid = (lo + hi) >> 1;
      if (ends[mid] > q) hi = mid; else lo = mid + 1;
    }
    bit = (lo & 1) != 0;
  }
  const unsigned long long bits = __ballot(bit);
  if (lane == 0) words_all[word_offsets[m] + word] = bits;
}

}  // namespace

extern "C" int ovis_coco_rle_count(const uint8_t* chars, const int64_t* char_offsets, int num, int32_t* num_runs,
                                   void* stream) {
  if (num < 0) return OVIS_EINVAL;
  if (num > 65535) return OVIS_ERANGE;
  if (num == 0) return OVIS_OK;
  if (!char_offsets || !num_runs) return OVIS_EINVAL;
  hipLaunchKernelGGL(coco_rle_count_kernel, dim3((unsigned)num), dim3(kDecThreads), 0, (hipStream_t)stream,
                     (const unsigned char*)chars, (const long*)char_offsets, num_runs);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}

extern "C" int ovis_coco_rle_runs(const uint8_t* chars, const int64_t* char_offsets, const int64_t* run_offsets, int num,
                                  int32_t* runs, int32_t* status, void* stream) {
  if (num < 0) return OVIS_EINVAL;
  if (num > 65535) return OVIS_ERANGE;
  if (num == 0) return OVIS_OK;
  if (!char_offsets || !run_offsets || !status) return OVIS_EINVAL;
  hipLaunchKernelGGL(coco_rle_runs_kernel, dim3((unsigned)num), dim3(kDecThreads), 0, (hipStream_t)stream,
                     (const unsigned char*)chars, (const long*)char_offsets, (const long*)run_offsets, runs, status);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}

extern "C" int ovis_coco_runs_to_words(const int32_t* runs, const int64_t* run_offsets, const int32_t* sizes,
                                       const int64_t* word_offsets, int num, long max_words, int32_t* run_ends,
                                       uint64_t* words, int64_t* areas, int32_t* status, void* stream) {
  if (num < 0 || max_words < 0) return OVIS_EINVAL;
  if (num > 65535 || max_words > (kDecMaxPixels + 63) / 64) return OVIS_ERANGE;
  if (num == 0) return OVIS_OK;
  if (!run_offsets || !sizes || !word_offsets || !areas || !status) return OVIS_EINVAL;
  hipLaunchKernelGGL(coco_run_ends_kernel, dim3((unsigned)num), dim3(kDecThreads), 0, (hipStream_t)stream, runs,
                     (const long*)run_offsets, sizes, run_ends, (long*)areas, status);
  OVIS_LAUNCH_CHECK();
  if (max_words == 0) return OVIS_OK;
  if (!words) return OVIS_EINVAL;
  hipLaunchKernelGGL(coco_words_kernel, dim3((unsigned)ovis_ceil_div(max_words, kDecWaves), (unsigned)num),
                     dim3(kDecThreads), 0, (hipStream_t)stream, run_ends, (const long*)run_offsets, sizes,
                     (const long*)word_offsets, status, (unsigned long long*)words);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}
