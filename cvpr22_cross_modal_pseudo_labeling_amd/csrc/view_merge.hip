// Merge of the detections of several test-time-augmentation views of a batch for gfx950 (MI355X).
//
// The reference (maskrcnn_benchmark/engine/bbox_aug.py:53-60 with structures/bounding_box.py:91-166 and the per-class loop
// of modeling/roi_heads/box_head/inference.py:121-163) maps every view's boxes back per view and per image with
// BoxList.transpose + BoxList.resize, concatenates them and then, per class, takes `nonzero(scores > thresh)` -- about ten
// small launches per view and a host sync per class.  Here three launches write the flipped-back, rescaled, thresholded,
// class-major candidate list of the WHOLE batch, in the order that loop would visit (image, class, segment = view, row):
//
//   view_merge_count_kernel   one workgroup per (64-row tile of a segment, chunk of 64 classes): the number of rows of the
//                             tile above the threshold, per class
//   exclusive_scan_kernel     one workgroup: the counts, laid out [image][class][tile of the image], become the start of
//                             every (image, class, tile) run; the total K lands in offsets[num_images * num_classes]
//   view_merge_scatter_kernel the same tiles again: a candidate's place is its run's start + its rank inside the tile (a
//                             wave64 ballot + popcount), so the placement is a pure function of the inputs -- no atomic
//                             counter, no dependence on scheduling (NMS breaks ties between equal scores by this order)
//
// scores is row-major [R, C] and the list is class-major: a wave reads 64 consecutive classes of one row (256 contiguous
// bytes), ballots them into one 64-bit word per row, and the 64 x 64 bit matrix is transposed through 512 bytes of LDS by
// a second round of ballots with the lanes on the rows.  Only the survivors' boxes and scores are read again (16-byte loads
// and stores).  The box arithmetic is BoxList.transpose(0) then BoxList.resize expression by expression (this library is
// built with -ffp-contract=off): x1' = (W - x2) - 1, x2' = (W - x1) - 1, then x * ratio_w, y * ratio_h.
#include "ovis_common.h"

namespace {

constexpr int kTileRows = OVIS_VIEW_MERGE_TILE_ROWS;  // = the wave width: one ballot bit per row
constexpr int kChunk = 64;                            // classes per workgroup: one ballot bit per class
static_assert(kTileRows == 64, "a tile is one wave64 ballot of rows");

struct MergeSegments {   // kernel argument: 10 x 64 words + 2 (2568 bytes)
  int count;
  int num_classes;
  int tile_start[OVIS_VIEW_MERGE_MAX_SEGMENTS];   // first tile of the segment among the launch's tiles (every segment has >= 1)
  int row_start[OVIS_VIEW_MERGE_MAX_SEGMENTS];
  int row_count[OVIS_VIEW_MERGE_MAX_SEGMENTS];
  int image[OVIS_VIEW_MERGE_MAX_SEGMENTS];
  int image_tile0[OVIS_VIEW_MERGE_MAX_SEGMENTS];  // first tile of the segment's image among the launch's tiles
  int image_tiles[OVIS_VIEW_MERGE_MAX_SEGMENTS];  // tiles of the segment's image
  int flip[OVIS_VIEW_MERGE_MAX_SEGMENTS];
  float width[OVIS_VIEW_MERGE_MAX_SEGMENTS];
  float ratio_w[OVIS_VIEW_MERGE_MAX_SEGMENTS];
  float ratio_h[OVIS_VIEW_MERGE_MAX_SEGMENTS];
};

struct Tile {
  int seg;
  long row0;   // first row of the tile in boxes / scores
  int rows;    // 0..64
  long entry0; // count entry of (class 0, this tile); class c is entry0 + c * entry_stride
  int entry_stride;
  bool first_of_image;
};

__device__ __forceinline__ Tile locate_tile(const MergeSegments& s, int t) {
  int g = 0;
  while (g + 1 < s.count && t >= s.tile_start[g + 1]) ++g;
  Tile tile;
  tile.seg = g;
  const int local = (t - s.tile_start[g]) * kTileRows;
  tile.row0 = (long)s.row_start[g] + local;
  const int left = s.row_count[g] - local;
  tile.rows = left < 0 ? 0 : (left > kTileRows ? kTileRows : left);
  tile.entry0 = (long)s.image_tile0[g] * s.num_classes + (t - s.image_tile0[g]);
  tile.entry_stride = s.image_tiles[g];
  tile.first_of_image = t == s.image_tile0[g];
  return tile;
}

// -> this lane's row (= lane) as a word of class bits: bit j set iff scores[row, c0 + j] > thresh, class >= 1.  256 threads.
__device__ __forceinline__ unsigned long long row_class_bits(const float* __restrict__ scores, const Tile& tile, int C, int c0,
                                                             float thresh, unsigned long long* row_bits) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = c0 + lane;
#pragma unroll 4
  for (int k = 0; k < kTileRows / 4; ++k) {
    const int r = wave * (kTileRows / 4) + k;      // wave-uniform
    bool pass = false;
    if (r < tile.rows && c < C && c >= 1) pass = scores[(tile.row0 + r) * (long)C + c] > thresh;  // a NaN is not kept
    const unsigned long long m = __ballot(pass);
    if (lane == 0) row_bits[r] = m;
  }
  __syncthreads();
  return row_bits[lane];
}

__global__ __launch_bounds__(256) void view_merge_count_kernel(const float* __restrict__ scores, MergeSegments segs,
                                                              float thresh, int* __restrict__ counts) {
  __shared__ unsigned long long row_bits[kTileRows];
  const int C = segs.num_classes, c0 = blockIdx.y * kChunk;
  const Tile tile = locate_tile(segs, blockIdx.x);
  const unsigned long long mine = row_class_bits(scores, tile, C, c0, thresh, row_bits);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kChunk / 4; ++k) {
    const int j = wave * (kChunk / 4) + k;
    const unsigned long long rows_of_class = __ballot(((mine >> j) & 1ull) != 0);
    if (lane == 0 && c0 + j < C) counts[tile.entry0 + (long)(c0 + j) * tile.entry_stride] = __popcll(rows_of_class);
  }
}

// in-place exclusive scan of n int32 by ONE workgroup, 1024 at a time with a running carry; *total = the sum
__global__ __launch_bounds__(1024) void exclusive_scan_kernel(int* __restrict__ data, long n, int* __restrict__ total) {
  __shared__ int wave_total[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;
  for (long base = 0; base < n; base += 1024) {
    const long i = base + threadIdx.x;
    const int v = i < n ? data[i] : 0;
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int up = __shfl_up(incl, off);
      if (lane >= off) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int s = wave_total[k];
      before += k < wave ? s : 0;
      all += s;
    }
    if (i < n) data[i] = carry + before + incl - v;
    carry += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(256) void view_merge_scatter_kernel(const float4* __restrict__ boxes,
                                                                const float* __restrict__ scores, MergeSegments segs,
                                                                float thresh, const int* __restrict__ starts,
                                                                long capacity, float4* __restrict__ cand_boxes,
                                                                float* __restrict__ cand_scores,
                                                                int* __restrict__ cand_group, int* __restrict__ offsets) {
  __shared__ unsigned long long row_bits[kTileRows];
  const int C = segs.num_classes, c0 = blockIdx.y * kChunk;
  const Tile tile = locate_tile(segs, blockIdx.x);
  const unsigned long long mine = row_class_bits(scores, tile, C, c0, thresh, row_bits);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = tile.seg;
  const int image = segs.image[g];
  const bool flip = segs.flip[g] != 0;
  const float W = segs.width[g], rw = segs.ratio_w[g], rh = segs.ratio_h[g];
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int k = 0; k < kChunk / 4; ++k) {
    const int j = wave * (kChunk / 4) + k;
    const int c = c0 + j;                          // wave-uniform
    const bool keep = ((mine >> j) & 1ull) != 0;
    const unsigned long long rows_of_class = __ballot(keep);
    if (c >= C) break;
    const int start = starts[tile.entry0 + (long)c * tile.entry_stride];
    if (tile.first_of_image && lane == 0) offsets[(long)image * C + c] = start;
    const long at = (long)start + __popcll(rows_of_class & below);
    if (keep && at < capacity) {                   // at >= capacity cannot happen with the counts of the same inputs
      const long src = (tile.row0 + lane) * (long)C + c;
      float4 b = boxes[src];
      if (flip) {                                  // BoxList.transpose(FLIP_LEFT_RIGHT): width - xmax - 1, width - xmin - 1
        const float x1 = (W - b.z) - 1.f, x2 = (W - b.x) - 1.f;
        b.x = x1;
        b.z = x2;
      }
      b.x = b.x * rw;                              // BoxList.resize
      b.y = b.y * rh;
      b.z = b.z * rw;
      b.w = b.w * rh;
      cand_boxes[at] = b;
      cand_scores[at] = scores[src];
      cand_group[at] = image * C + c;
    }
  }
}

// the segment records of one launch (HOST arrays) -> the kernel argument; *tiles = the launch's tile count
int fill_segments(long num_rows, int num_classes, int num_images, const int32_t* segments, const float* ratios,
                  int num_segments, MergeSegments* out, long* tiles) {
  if (num_rows < 0 || num_classes < 1 || num_images < 0 || num_segments < 1) return OVIS_EINVAL;
  if (num_segments > OVIS_VIEW_MERGE_MAX_SEGMENTS) return OVIS_ERANGE;
  if (!segments || !ratios) return OVIS_EINVAL;
  if ((double)num_rows * num_classes > 2147483647.0 || (double)num_images * num_classes >= 2147483647.0) return OVIS_ERANGE;
  out->count = num_segments;
  out->num_classes = num_classes;
  long t = 0;
  int first = 0;  // first segment of the current image
  for (int g = 0; g < num_segments; ++g) {
    const int32_t* rec = segments + 5 * g;  // row_start, row_count, image, view_width, flip
    if (rec[0] < 0 || rec[1] < 0 || (long)rec[0] + rec[1] > num_rows) return OVIS_EINVAL;  // never read outside scores / boxes
    if (rec[2] < 0 || rec[2] >= num_images || rec[3] < 0) return OVIS_EINVAL;
    if (g > 0 && (rec[2] < segments[5 * (g - 1) + 2] || rec[2] > segments[5 * (g - 1) + 2] + 1))
      return OVIS_EINVAL;                   // image-major, and every image of the call's range owns a segment
    if (g > 0 && rec[2] != segments[5 * (g - 1) + 2]) {
      for (int k = first; k < g; ++k) out->image_tiles[k] = (int)t - out->image_tile0[k];
      first = g;
    }
    out->tile_start[g] = (int)t;
    out->image_tile0[g] = g == first ? (int)t : out->image_tile0[first];
    out->row_start[g] = rec[0];
    out->row_count[g] = rec[1];
    out->image[g] = rec[2];
    out->width[g] = (float)rec[3];
    out->flip[g] = rec[4] != 0;
    out->ratio_w[g] = ratios[2 * g];
    out->ratio_h[g] = ratios[2 * g + 1];
    const long n = (rec[1] + kTileRows - 1) / kTileRows;
    t += n > 0 ? n : 1;   // an empty segment keeps one (empty) tile: every image owns count entries
  }
  for (int k = first; k < num_segments; ++k) out->image_tiles[k] = (int)t - out->image_tile0[k];
  for (int g = num_segments; g < OVIS_VIEW_MERGE_MAX_SEGMENTS; ++g) {
    out->tile_start[g] = (int)t;
    out->row_start[g] = out->row_count[g] = out->image[g] = out->image_tile0[g] = out->image_tiles[g] = out->flip[g] = 0;
    out->width[g] = out->ratio_w[g] = out->ratio_h[g] = 0.f;
  }
  *tiles = t;
  return OVIS_OK;
}

}  // namespace

extern "C" int ovis_view_merge_count_f32(const float* scores, long num_rows, int num_classes, int num_images,
                                         const int32_t* segments, const float* ratios, int num_segments,
                                         float score_thresh, int32_t* counts, long num_counts, void* stream) {
  MergeSegments segs;
  long tiles = 0;
  const int rc = fill_segments(num_rows, num_classes, num_images, segments, ratios, num_segments, &segs, &tiles);
  if (rc != OVIS_OK) return rc;
  if (!counts || num_counts != tiles * num_classes || (num_rows > 0 && !scores)) return OVIS_EINVAL;
  const int chunks = ovis_ceil_div(num_classes, kChunk);
  if (chunks > 65535) return OVIS_ERANGE;
  hipLaunchKernelGGL(view_merge_count_kernel, dim3((unsigned)tiles, chunks), dim3(256), 0, (hipStream_t)stream, scores, segs,
                     score_thresh, counts);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}

extern "C" int ovis_view_merge_scan_i32(int32_t* counts, long num_counts, int32_t* total, void* stream) {
  if (num_counts < 0 || !total || (num_counts > 0 && !counts)) return OVIS_EINVAL;
  hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, counts, num_counts, total);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}

extern "C" int ovis_view_merge_scatter_f32(const float* boxes, const float* scores, long num_rows, int num_classes,
                                           int num_images, const int32_t* segments, const float* ratios, int num_segments,
                                           float score_thresh, const int32_t* starts, long num_counts,
                                           long num_candidates, float* cand_boxes, float* cand_scores, int32_t* cand_group,
                                           int32_t* offsets, void* stream) {
  MergeSegments segs;
  long tiles = 0;
  const int rc = fill_segments(num_rows, num_classes, num_images, segments, ratios, num_segments, &segs, &tiles);
  if (rc != OVIS_OK) return rc;
  if (!starts || !offsets || num_counts != tiles * num_classes || num_candidates < 0) return OVIS_EINVAL;
  if (num_rows > 0 && (!scores || !boxes || ((uintptr_t)boxes & 15) != 0)) return OVIS_EINVAL;
  if (num_candidates > 0 && (!cand_boxes || !cand_scores || !cand_group || ((uintptr_t)cand_boxes & 15) != 0)) return OVIS_EINVAL;
  const int chunks = ovis_ceil_div(num_classes, kChunk);
  if (chunks > 65535) return OVIS_ERANGE;
  hipLaunchKernelGGL(view_merge_scatter_kernel, dim3((unsigned)tiles, chunks), dim3(256), 0, (hipStream_t)stream,
                     (const float4*)boxes, scores, segs, score_thresh, starts, num_candidates, (float4*)cand_boxes,
                     cand_scores, cand_group, offsets);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}
