// Mask targets straight from the bit words of RLE ground truth (csrc/coco_rle_decode.hip): the chain the reference runs on a
// SegmentationMask(mode='mask') -- BinaryMaskList.resize to the training size, .transpose for the flips
// (structures/segmentation_mask.py:138-156, 113-116), then project_masks_on_boxes (mask_head/loss.py:11-42: .crop to the
// rounded box :117-136, .resize to M x M) -- without ever writing the h1 x w1 canvas.
//
// A uint8 mask that is resampled bilinearly and truncated is 1 where the interpolated value reaches 1.0: where EVERY tap
// with a non-zero weight is set.  That is the rule here, on both resizes (the reference's fp32 sum departs from it by a
// rounding in a few per cent of the M x M pixels; README "RLE ground truth"):
//
//   R[y][x] = S[y0][x0] & (lx == 0 | S[y0][x1]) & (ly == 0 | S[y1][x0]) & (lx == 0 | ly == 0 | S[y1][x1])
//
// with the taps (i0, i1, lam) of mask_axis_tap (mask_crop_geom.h), the expressions of project_masks_kernel.  Chain: S the
// decoded h0 x w0 bitmap; R = the rule h0 x w0 -> h1 x w1; F = R flipped; the crop window of mask_crop_window on (w1, h1);
// the rule again ch x cw -> M x M on F.  An output pixel is 4 pixels of F x 4 bits of S.
//
//   project_rle_masks_kernel   one workgroup per positive.  The first 2 * M lanes build the per-axis tap tables in LDS: for
//                              each of the M output rows / columns its two positions in F and, for each of them (un-flipped),
//                              the two source positions, plus the three "second weight is zero" flags.  Then every lane
//                              does the bit tests of its outputs; nothing but the tables depends on the geometry.
//
// ADDRESSING.  Pixel (y, x) of a mask is bit (y * w0 + x) & 63 of word (y * w0 + x) >> 6 of its slice.  A slice is read only
// when word_offsets gives it exactly ceil(h0 * w0 / 64) words, and y < h0, x < w0 by the taps' clamps, so every load is
// inside the slice; gt_index and instance are checked against their counts.  A word's bits are tested, never used as an
// address (the rule at the top of coco_rle_decode.hip).  No atomics; every output is written once.
#include "ovis_common.h"
#define OVIS_HD __device__ __forceinline__
#include "mask_crop_geom.h"

namespace {

constexpr int kRleThreads = 256;
constexpr int kRleMaxRes = kRleThreads / 2;     // one lane per table row of either axis
constexpr long kRleMaxPixels = 0x7fffffefL;     // the decoder's bound (csrc/coco_rle_decode.hip)
constexpr int kRleMaxSide = 1 << 24;            // sizes are exact in fp32

__global__ __launch_bounds__(kRleThreads) void project_rle_masks_kernel(
    const unsigned long long* __restrict__ words, const long* __restrict__ word_offsets, int num_masks,
    const long* __restrict__ instance, int num_instances, const long* __restrict__ gt_index, const float* __restrict__ boxes,
    int h0, int w0, int h1, int w1, int flip_h, int flip_v, int M, long words_per_mask, float* __restrict__ out) {
  // [axis 0 = y, 1 = x][output index]: src = {S taps of F position 0, S taps of F position 1}; zero = bit 0: the second
  // F position has no weight, bits 1 / 2: the second S tap of F position 0 / 1 has no weight
  __shared__ int src[2][kRleMaxRes][4];
  __shared__ int zero[2][kRleMaxRes];
  const int p = blockIdx.x, tid = threadIdx.x;
  if (tid < 2 * M) {
    const int axis = tid / M, d = tid - axis * M;
    const MaskCropWindow c = mask_crop_window(*(const float4*)(boxes + 4 * p), w1, h1);
    const int n0 = axis ? w0 : h0, n1 = axis ? w1 : h1, flip = axis ? flip_h : flip_v;
    const float lo = axis ? c.xmin : c.ymin;
    const MaskAxisTap t2 = mask_axis_tap(d, axis ? c.w : c.h, (float)M);
    int z = t2.lam == 0.f ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      int f = (int)((k ? t2.i1 : t2.i0) + lo);   // a position of the crop in F: inside [0, n1 - 1]
      f = min(max(f, 0), n1 - 1);
      const int r = flip ? n1 - 1 - f : f;       // the same pixel before the flip
      const MaskAxisTap t1 = mask_axis_tap(r, (float)n0, (float)n1);
      src[axis][d][2 * k] = min(max((int)t1.i0, 0), n0 - 1);
      src[axis][d][2 * k + 1] = min(max((int)t1.i1, 0), n0 - 1);
      z |= t1.lam == 0.f ? 2 << k : 0;
    }
    zero[axis][d] = z;
  }
  __syncthreads();
  // the positive's mask: its slice of the words, or nothing (all targets 0) when an index or the slice's size is off
  const long g = gt_index[p];
  const long m = g >= 0 && g < num_instances ? instance[g] : -1;
  const bool known = m >= 0 && m < num_masks;
  const long begin = known ? word_offsets[m] : 0;
  const bool good = known && word_offsets[m + 1] - begin == words_per_mask;
  const unsigned long long* mask = words + begin;
  auto bit = [&](int y, int x) -> bool {   // y < h0, x < w0: the bit is inside the slice's words_per_mask words
    const long q = (long)y * w0 + x;
    return (mask[q >> 6] >> (q & 63)) & 1ull;
  };
  // pixel (ky, kx) of the four pixels of F an output reads: the rule on S
  auto resized = [&](const int* sy, int zy, int ky, const int* sx, int zx, int kx) -> bool {
    const int y0 = sy[2 * ky], y1 = sy[2 * ky + 1], x0 = sx[2 * kx], x1 = sx[2 * kx + 1];
    const bool ny = (zy >> (1 + ky)) & 1, nx = (zx >> (1 + kx)) & 1;
    return bit(y0, x0) && (nx || bit(y0, x1)) && (ny || bit(y1, x0)) && (nx || ny || bit(y1, x1));
  };
  float* o = out + (long)p * M * M;
  for (int i = tid; i < M * M; i += kRleThreads) {
    const int dy = i / M, dx = i - dy * M;
    bool v = false;
    if (good) {
      const int* sy = src[0][dy];
      const int* sx = src[1][dx];
      const int zy = zero[0][dy], zx = zero[1][dx];
      const bool ny = zy & 1, nx = zx & 1;
      v = resized(sy, zy, 0, sx, zx, 0) && (nx || resized(sy, zy, 0, sx, zx, 1)) && (ny || resized(sy, zy, 1, sx, zx, 0)) &&
          (nx || ny || resized(sy, zy, 1, sx, zx, 1));
    }
    o[i] = v ? 1.f : 0.f;
  }
}

// The same chain with ONE integer window between the flips and the box crop (RleMasks.crop behind the input transform's
// scale jitter): the mask the box is cropped from is F[win_y : win_y + win_h, win_x : win_x + win_w].  The box is rounded and
// clamped in the WINDOW's frame (mask_crop_window on (win_w, win_h)) and the integer offset is added to the positions
// afterwards -- cropping a canvas, then cropping it again; rounding box + offset differs when the box lands on a .5 and the
// offset is odd (half to even).  Only the table build differs from project_rle_masks_kernel, which stays as it is; with the
// window equal to the frame the tables, and so the output, are the same.
__global__ __launch_bounds__(kRleThreads) void project_rle_masks_window_kernel(
    const unsigned long long* __restrict__ words, const long* __restrict__ word_offsets, int num_masks,
    const long* __restrict__ instance, int num_instances, const long* __restrict__ gt_index, const float* __restrict__ boxes,
    int h0, int w0, int h1, int w1, int flip_h, int flip_v, int win_y, int win_x, int win_h, int win_w, int M,
    long words_per_mask, float* __restrict__ out) {
  __shared__ int src[2][kRleMaxRes][4];
  __shared__ int zero[2][kRleMaxRes];
  const int p = blockIdx.x, tid = threadIdx.x;
  if (tid < 2 * M) {
    const int axis = tid / M, d = tid - axis * M;
    const MaskCropWindow c = mask_crop_window(*(const float4*)(boxes + 4 * p), win_w, win_h);
    const int n0 = axis ? w0 : h0, n1 = axis ? w1 : h1, flip = axis ? flip_h : flip_v;
    const int nw = axis ? win_w : win_h, off = axis ? win_x : win_y;
    const float lo = axis ? c.xmin : c.ymin;
    const MaskAxisTap t2 = mask_axis_tap(d, axis ? c.w : c.h, (float)M);
    int z = t2.lam == 0.f ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      int f = (int)((k ? t2.i1 : t2.i0) + lo);   // a position of the crop in the window: inside [0, nw - 1]
      f = min(max(f, 0), nw - 1) + off;          // the same pixel in F: off + nw <= n1 (checked by the entry point)
      const int r = flip ? n1 - 1 - f : f;       // and before the flip
      const MaskAxisTap t1 = mask_axis_tap(r, (float)n0, (float)n1);
      src[axis][d][2 * k] = min(max((int)t1.i0, 0), n0 - 1);
      src[axis][d][2 * k + 1] = min(max((int)t1.i1, 0), n0 - 1);
      z |= t1.lam == 0.f ? 2 << k : 0;
    }
    zero[axis][d] = z;
  }
  __syncthreads();
  const long g = gt_index[p];
  const long m = g >= 0 && g < num_instances ? instance[g] : -1;
  const bool known = m >= 0 && m < num_masks;
  const long begin = known ? word_offsets[m] : 0;
  const bool good = known && word_offsets[m + 1] - begin == words_per_mask;
  const unsigned long long* mask = words + begin;
  auto bit = [&](int y, int x) -> bool {   // y < h0, x < w0: the bit is inside the slice's words_per_mask words
    const long q = (long)y * w0 + x;
    return (mask[q >> 6] >> (q & 63)) & 1ull;
  };
  auto resized = [&](const int* sy, int zy, int ky, const int* sx, int zx, int kx) -> bool {
    const int y0 = sy[2 * ky], y1 = sy[2 * ky + 1], x0 = sx[2 * kx], x1 = sx[2 * kx + 1];
    const bool ny = (zy >> (1 + ky)) & 1, nx = (zx >> (1 + kx)) & 1;
    return bit(y0, x0) && (nx || bit(y0, x1)) && (ny || bit(y1, x0)) && (nx || ny || bit(y1, x1));
  };
  float* o = out + (long)p * M * M;
  for (int i = tid; i < M * M; i += kRleThreads) {
    const int dy = i / M, dx = i - dy * M;
    bool v = false;
    if (good) {
      const int* sy = src[0][dy];
      const int* sx = src[1][dx];
      const int zy = zero[0][dy], zx = zero[1][dx];
      const bool ny = zy & 1, nx = zx & 1;
      v = resized(sy, zy, 0, sx, zx, 0) && (nx || resized(sy, zy, 0, sx, zx, 1)) && (ny || resized(sy, zy, 1, sx, zx, 0)) &&
          (nx || ny || resized(sy, zy, 1, sx, zx, 1));
    }
    o[i] = v ? 1.f : 0.f;
  }
}

}  // namespace

extern "C" int ovis_project_rle_masks_window_f32(const uint64_t* words, const int64_t* word_offsets, int num_masks,
                                                 long words_per_mask, const int64_t* instance, int num_instances,
                                                 const int64_t* gt_index, const float* boxes, int num, int h0, int w0,
                                                 int h1, int w1, int flip_h, int flip_v, int win_y, int win_x, int win_h,
                                                 int win_w, int resolution, float* out, void* stream) {
  if (num < 0 || num_masks < 0 || num_instances < 0 || h0 <= 0 || w0 <= 0 || h1 <= 0 || w1 <= 0 || resolution <= 0)
    return OVIS_EINVAL;
  if (resolution > kRleMaxRes || h0 > kRleMaxSide || w0 > kRleMaxSide || h1 > kRleMaxSide || w1 > kRleMaxSide ||
      (long)h0 * w0 > kRleMaxPixels || words_per_mask != ((long)h0 * w0 + 63) / 64)
    return OVIS_ERANGE;
  if (win_y < 0 || win_x < 0 || win_h < 1 || win_w < 1 || win_h > h1 - win_y || win_w > w1 - win_x) return OVIS_EINVAL;
  if (num == 0) return OVIS_OK;
  if (!words || !word_offsets || !instance || !gt_index || !boxes || !out) return OVIS_EINVAL;
  if ((uintptr_t)boxes & 15) return OVIS_ERANGE;
  hipLaunchKernelGGL(project_rle_masks_window_kernel, dim3((unsigned)num), dim3(kRleThreads), 0, (hipStream_t)stream,
                     (const unsigned long long*)words, (const long*)word_offsets, num_masks, (const long*)instance,
                     num_instances, (const long*)gt_index, boxes, h0, w0, h1, w1, flip_h ? 1 : 0, flip_v ? 1 : 0, win_y, win_x,
                     win_h, win_w, resolution, words_per_mask, out);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}

extern "C" int ovis_project_rle_masks_f32(const uint64_t* words, const int64_t* word_offsets, int num_masks,
                                          long words_per_mask, const int64_t* instance, int num_instances,
                                          const int64_t* gt_index, const float* boxes, int num, int h0, int w0, int h1,
                                          int w1, int flip_h, int flip_v, int resolution, float* out, void* stream) {
  if (num < 0 || num_masks < 0 || num_instances < 0 || h0 <= 0 || w0 <= 0 || h1 <= 0 || w1 <= 0 || resolution <= 0)
    return OVIS_EINVAL;
  if (resolution > kRleMaxRes || h0 > kRleMaxSide || w0 > kRleMaxSide || h1 > kRleMaxSide || w1 > kRleMaxSide ||
      (long)h0 * w0 > kRleMaxPixels || words_per_mask != ((long)h0 * w0 + 63) / 64)
    return OVIS_ERANGE;
  if (num == 0) return OVIS_OK;
  if (!words || !word_offsets || !instance || !gt_index || !boxes || !out) return OVIS_EINVAL;
  if ((uintptr_t)boxes & 15) return OVIS_ERANGE;
  hipLaunchKernelGGL(project_rle_masks_kernel, dim3((unsigned)num), dim3(kRleThreads), 0, (hipStream_t)stream,
                     (const unsigned long long*)words, (const long*)word_offsets, num_masks, (const long*)instance,
                     num_instances, (const long*)gt_index, boxes, h0, w0, h1, w1, flip_h ? 1 : 0, flip_v ? 1 : 0, resolution,
                     words_per_mask, out);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}
