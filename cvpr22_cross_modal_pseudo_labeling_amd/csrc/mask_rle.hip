// COCO run-length encodings of pasted masks, straight from (M x M probability map, box, image size) triples: what the
// reference gets by pasting every mask into an H x W canvas, copying it to the host and calling pycocotools' encode
// (data/datasets/evaluation/coco/coco_eval.py:112-144 over mask_head/inference.py:100-205).  The canvas is never built:
// a pixel is pasted_inside() of pasted_geom.h -- the expression sequence of paste_masks_kernel (csrc/paste.hip), so the
// decoded runs equal its bytes -- and everything outside the integer box clipped to the image is zero.
//
// The runs are pycocotools' rleEncode: the mask in column-major order, v(j) for j = x * H + y with v(-1) = 0; a run ENDS
// at every j with v(j) != v(j - 1); counts are the gaps between consecutive ends, from 0 up to H * W.  Only a pixel of the
// clipped box, or the pixel behind a column of the box in linear order, can be an end.  A lane owns one column x of the
// box and walks its rows:
//   * its `previous` starts at 0 -- unless the box touches the top AND the bottom row and x is not its first column: then
//     the pixel in front of (x, 0) is (x - 1, H - 1) of the box, and a run may go on across the column boundary;
//   * behind the column's last row comes j = x * H + cy1 + 1 (pixel (x, cy1 + 1), or (x + 1, 0) when cy1 = H - 1).  It
//     exists unless this is the image's last pixel; it is zero unless it is the box's own (x + 1, 0), which the NEXT
//     column's walk judges as above.  So a set last pixel ends a run there in every other case.
// The order of the ends is the order of the columns, then of the rows: a workgroup scan over the columns' end counts
// (carried from round to round when the box is wider than the workgroup) gives every column its first slot.  No atomics.
//
//   pasted_rle_count_kernel   one workgroup per mask: the number of counts (ends + 1), or -1 for an unusable image size
//   pasted_rle_runs_kernel    the same walk twice per round (count, scan, store): the ends at their slots, then -- in
//                             place, the workgroup owns the mask's slots -- the differences, and the length of the
//                             compressed string
//   pasted_rle_string_kernel  pycocotools' rleToString: characters per count, the same scan, the bytes
#include "ovis_common.h"
#define OVIS_HD __device__ __forceinline__
#include "pasted_geom.h"

namespace {

constexpr int kRleThreads = 256;
constexpr int kRleWaves = kRleThreads / OVIS_WAVE;
constexpr int kRleMaxM = 120;              // (M + 2)^2 floats of LDS <= 64 KB, as csrc/paste.hip
constexpr long kRleMaxPixels = 0x7fffffefL;  // x * H + y fits in a signed 32-bit word, as csrc/paste.hip

// exclusive prefix of v over the workgroup's lanes in thread order; *total = the sum.  Ends with a barrier in front of
// which every lane has read wave_total, so the caller may use it again at once.
__device__ __forceinline__ int block_exclusive_scan(int v, int* wave_total, int* total) {
  const int lane = threadIdx.x & (OVIS_WAVE - 1), wave = threadIdx.x / OVIS_WAVE;
  int incl = v;
#pragma unroll
  for (int off = 1; off < OVIS_WAVE; off <<= 1) {
    const int up = __shfl_up(incl, off);
    if (lane >= off) incl += up;
  }
  if (lane == OVIS_WAVE - 1) wave_total[wave] = incl;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < kRleWaves; ++k) {
    const int s = wave_total[k];
    before += k < wave ? s : 0;
    all += s;
  }
  __syncthreads();
  *total = all;
  return before + incl - v;
}

// One mask's geometry and its zero-padded map in LDS.
struct PastedMask {
  const float* padded;  // [(M+2), (M+2)]
  int M, H, W;
  int4 bx;
  int bw, bh;
  float thr;
  int cx0, cx1, cy0, cy1;  // the integer box clipped to the image (inclusive; empty when c?1 < c?0)

  __device__ __forceinline__ bool pixel(int y, int x) const {  // (y, x) inside the clipped box
    const int S = M + 2;
    const float* pd = padded;
    auto at = [pd, S](int yy, int xx) { return pd[yy * S + xx]; };
    return pasted_inside(at, M, bx, bw, bh, thr, y, x);
  }
  // columns of the clipped box; 0 when it misses the image or is degenerate.  A long: W may be close to 2^31
  __device__ __forceinline__ long columns() const { return cx1 < cx0 || cy1 < cy0 ? 0 : (long)cx1 - cx0 + 1; }
  __device__ __forceinline__ bool full_height() const { return cy0 == 0 && cy1 == H - 1; }
};

// false: the image size is unusable (nothing else of *m is set then).  Every lane of the workgroup calls this.
__device__ __forceinline__ bool load_mask(const float* __restrict__ probs, const float* __restrict__ boxes,
                                          const int* __restrict__ sizes, int M, float thr, float* padded, PastedMask* m) {
  const int p = blockIdx.x;
  const int H = sizes[2 * p], W = sizes[2 * p + 1];
  if (H < 1 || W < 1 || (long)H * W > kRleMaxPixels) return false;
  const int S = M + 2;
  const float* pr = probs + (long)p * M * M;
  for (int i = threadIdx.x; i < S * S; i += kRleThreads) {
    const int y = i / S, x = i - y * S;
    padded[i] = (y >= 1 && y <= M && x >= 1 && x <= M) ? pr[(y - 1) * M + (x - 1)] : 0.f;
  }
  __syncthreads();
  const PastedBox pb = pasted_box(*(const float4*)(boxes + 4 * (long)p), M);
  m->padded = padded;
  m->M = M;
  m->H = H;
  m->W = W;
  m->bx = pb.bx;
  m->bw = pb.bw;
  m->bh = pb.bh;
  m->thr = thr;
  m->cx0 = max(pb.bx.x, 0);
  m->cx1 = min(pb.bx.z, W - 1);
  m->cy0 = max(pb.bx.y, 0);
  m->cy1 = min(pb.bx.w, H - 1);
  return true;
}

// The run ends column x of the clipped box contributes, in order: end(j, k) for the k-th at linear index j; -> their number.
template <typename End>
__device__ __forceinline__ int walk_column(const PastedMask& m, int x, End&& end) {
  const bool full = m.full_height();
  bool prev = full && x > m.cx0 && m.pixel(m.H - 1, x - 1);
  int n = 0;
  const int j0 = x * m.H;
  for (int y = m.cy0; y <= m.cy1; ++y) {
    const bool v = m.pixel(y, x);
    if (v != prev) {
      end(j0 + y, n);
      ++n;
    }
    prev = v;
  }
  const bool last_of_image = m.cy1 == m.H - 1 && x == m.W - 1;
  const bool next_is_own = full && x < m.cx1;
  if (prev && !last_of_image && !next_is_own) {
    end(j0 + m.cy1 + 1, n);
    ++n;
  }
  return n;
}

__global__ __launch_bounds__(kRleThreads) void pasted_rle_count_kernel(const float* __restrict__ probs,
                                                                      const float* __restrict__ boxes,
                                                                      const int* __restrict__ sizes, int M, float thr,
                                                                      int* __restrict__ num_runs) {
  extern __shared__ float padded[];
  __shared__ int wave_total[kRleWaves];
  PastedMask m;
  if (!load_mask(probs, boxes, sizes, M, thr, padded, &m)) {
    if (threadIdx.x == 0) num_runs[blockIdx.x] = -1;
    return;
  }
  int n = 0;
  for (long c = threadIdx.x; c < m.columns(); c += kRleThreads) n += walk_column(m, m.cx0 + (int)c, [](int, int) {});
  int ends;
  block_exclusive_scan(n, wave_total, &ends);
  if (threadIdx.x == 0) num_runs[blockIdx.x] = ends + 1;
}

// count i of `runs` as rleToString writes it -> the number of characters (at most 7: 31 bits and a sign in groups of 5),
// *text = the characters, the first in the low byte
__device__ __forceinline__ int rle_chars(const int* runs, int i, unsigned long long* text) {
  int x = runs[i] - (i > 2 ? runs[i - 2] : 0);  // |x| < 2^31: both are counts of one image
  int n = 0;
  unsigned long long t = 0;
  bool more = true;
  while (more) {
    int ch = x & 0x1f;
    x >>= 5;  // arithmetic
    more = (ch & 0x10) ? x != -1 : x != 0;
    if (more) ch |= 0x20;
    t |= (unsigned long long)(ch + 48) << (8 * n);
    ++n;
  }
  *text = t;
  return n;
}

__global__ __launch_bounds__(kRleThreads) void pasted_rle_runs_kernel(const float* __restrict__ probs,
                                                                     const float* __restrict__ boxes,
                                                                     const int* __restrict__ sizes, int M, float thr,
                                                                     const long* __restrict__ offsets, int* runs_all,
                                                                     int* __restrict__ num_chars) {
  extern __shared__ float padded[];
  __shared__ int wave_total[kRleWaves];
  const int p = blockIdx.x, tid = threadIdx.x;
  PastedMask m;
  if (!load_mask(probs, boxes, sizes, M, thr, padded, &m)) return;
  int* runs = runs_all + offsets[p];
  const int n = (int)(offsets[p + 1] - offsets[p]);  // the counts this mask may write: the count kernel's ends + 1
  if (n < 1) return;
  // 1. the ends e_0 < e_1 < ... at slots 0 .. n - 2, H * W at slot n - 1
  int carry = 0;
  for (long c0 = 0; c0 < m.columns(); c0 += kRleThreads) {  // workgroup-uniform
    const bool has = c0 + tid < m.columns();
    const int x = m.cx0 + (int)(has ? c0 + tid : 0);
    const int mine = has ? walk_column(m, x, [](int, int) {}) : 0;
    int round_total;
    const int first = carry + block_exclusive_scan(mine, wave_total, &round_total);
    if (mine)
      walk_column(m, x, [&](int j, int k) {
        if (first + k < n - 1) runs[first + k] = j;  // beyond cannot happen with the count of the same inputs
      });
    carry += round_total;
  }
  if (tid == 0) runs[n - 1] = m.H * m.W;
  __syncthreads();
  // 2. counts[k] = e_k - e_(k-1), e_(-1) = 0, in place: blocks of slots from the top down, so the slot below a block is
  //    still an end when the block reads it; inside a block every lane reads before any writes
  for (int base = ((n - 1) / kRleThreads) * kRleThreads; base >= 0; base -= kRleThreads) {
    const int k = base + tid;
    int d = 0;
    if (k < n) d = runs[k] - (k > 0 ? runs[k - 1] : 0);
    __syncthreads();
    if (k < n) runs[k] = d;
  }
  if (!num_chars) return;
  __syncthreads();
  // 3. the length of the compressed string
  int chars = 0;
  unsigned long long text;
  for (int k = tid; k < n; k += kRleThreads) chars += rle_chars(runs, k, &text);
  int total;
  block_exclusive_scan(chars, wave_total, &total);
  if (tid == 0) num_chars[p] = total;
}

__global__ __launch_bounds__(kRleThreads) void pasted_rle_string_kernel(const int* __restrict__ runs_all,
                                                                       const long* __restrict__ run_offsets,
                                                                       const long* __restrict__ char_offsets,
                                                                       unsigned char* __restrict__ out_all) {
  __shared__ int wave_total[kRleWaves];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int* runs = runs_all + run_offsets[p];
  const int n = (int)(run_offsets[p + 1] - run_offsets[p]);
  unsigned char* out = out_all + char_offsets[p];
  const long room = char_offsets[p + 1] - char_offsets[p];
  long carry = 0;
  for (int base = 0; base < n; base += kRleThreads) {  // workgroup-uniform
    const int k = base + tid;
    unsigned long long text = 0;
    const int len = k < n ? rle_chars(runs, k, &text) : 0;
    int round_total;
    const long at = carry + block_exclusive_scan(len, wave_total, &round_total);
    for (int u = 0; u < len; ++u)
      if (at + u < room) out[at + u] = (unsigned char)(text >> (8 * u));  // beyond cannot happen with the lengths of the same runs
    carry += round_total;
  }
}

int check_masks(const void* probs, const void* boxes, const void* sizes, int num, int M) {
  if (num < 0 || M <= 0) return OVIS_EINVAL;
  if (M > kRleMaxM || num > 65535) return OVIS_ERANGE;
  if (num == 0) return OVIS_OK;
  if (!probs || !boxes || !sizes) return OVIS_EINVAL;
  if ((uintptr_t)boxes & 15) return OVIS_ERANGE;
  return OVIS_OK;
}

}  // namespace

extern "C" int ovis_pasted_rle_count(const float* mask_probs, const float* boxes, const int32_t* image_sizes, int num,
                                     int prob_resolution, float threshold, int32_t* num_runs, void* stream) {
  const int rc = check_masks(mask_probs, boxes, image_sizes, num, prob_resolution);
  if (rc != OVIS_OK || num == 0) return rc;
  if (!num_runs) return OVIS_EINVAL;
  const int S = prob_resolution + 2;
  hipLaunchKernelGGL(pasted_rle_count_kernel, dim3((unsigned)num), dim3(kRleThreads), sizeof(float) * S * S,
                     (hipStream_t)stream, mask_probs, boxes, image_sizes, prob_resolution, threshold, num_runs);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}

extern "C" int ovis_pasted_rle_runs(const float* mask_probs, const float* boxes, const int32_t* image_sizes, int num,
                                    int prob_resolution, float threshold, const int64_t* run_offsets, int32_t* runs,
                                    int32_t* num_chars, void* stream) {
  const int rc = check_masks(mask_probs, boxes, image_sizes, num, prob_resolution);
  if (rc != OVIS_OK || num == 0) return rc;
  if (!run_offsets || !runs) return OVIS_EINVAL;
  const int S = prob_resolution + 2;
  hipLaunchKernelGGL(pasted_rle_runs_kernel, dim3((unsigned)num), dim3(kRleThreads), sizeof(float) * S * S,
                     (hipStream_t)stream, mask_probs, boxes, image_sizes, prob_resolution, threshold,
                     (const long*)run_offsets, runs, num_chars);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}

extern "C" int ovis_pasted_rle_string(const int32_t* runs, const int64_t* run_offsets, const int64_t* char_offsets, int num,
                                      uint8_t* out, void* stream) {
  if (num < 0) return OVIS_EINVAL;
  if (num > 65535) return OVIS_ERANGE;
  if (num == 0) return OVIS_OK;
  if (!runs || !run_offsets || !char_offsets || !out) return OVIS_EINVAL;
  hipLaunchKernelGGL(pasted_rle_string_kernel, dim3((unsigned)num), dim3(kRleThreads), 0, (hipStream_t)stream, runs,
                     run_offsets, char_offsets, (unsigned char*)out);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}
