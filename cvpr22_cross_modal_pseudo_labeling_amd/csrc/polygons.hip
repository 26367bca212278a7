// Polygon ground-truth masks -> mask-head targets on the device, gfx950 (MI355X).
//
// Reference path: maskrcnn_benchmark/modeling/roi_heads/mask_head/loss.py:11-42 (project_masks_on_boxes) on
// SegmentationMask(mode='poly') targets: per positive proposal
//     PolygonInstance.crop(box)      structures/segmentation_mask.py:270-296   clamp the box (python floats), p -= (xmin, ymin)
//     PolygonInstance.resize((M,M))  :298-324                                  p *= M / w, M / h   (float32 tensors)
//     convert_to_binarymask()        :326-334    pycocotools.mask.frPyObjects -> merge -> decode at M x M
// The rasteriser lives in a third-party dependency that is NOT under /root/reference: pycocotools==2.0
// (requirements.txt:35), common/maskApi.c -- rleFrPoly (polygon -> RLE), rleMerge (union), rleDecode.  Its published
// algorithm is restated here (and in oracle/ovis_oracle.c, which this kernel is tested against bit for bit):
//   1. vertices are scaled by 5 and rounded ((int)(5 * v + .5), truncation) -- double arithmetic on the float32 inputs;
//   2. every edge is walked densely along its major axis: d = 0 .. max(|dx|, |dy|), the minor coordinate
//      (int)(start + slope * t + .5), points emitted from the edge's first vertex to its second;
//   3. wherever consecutive points differ in x, a boundary point is emitted at xd = (min-side x + .5) / 5 - .5 if that is
//      an integer column inside [0, w - 1], yd = ceil(clamp((min(y, y_prev) + .5) / 5 - .5, 0, h));
//   4. the boundary points' column-major positions x * h + y, sorted, are the run boundaries of the RLE; equal positions
//      cancel.  Decoded, pixel (x, y) is set iff an ODD number of boundary points lie at positions <= x * h + y.
// Step 4 is evaluated as "toggle a counter per position, then prefix parity", which needs no sort.  Polygons of one
// instance are merged by union (rleMerge, intersect = 0).
//
// One wave per positive proposal; its lanes share the points of an edge; toggles are LDS integer atomics; the prefix
// parity is a wave scan.  Nothing here is bandwidth: a step has <= 512 positives of ~10-100 vertices each.
#include "ovis_common.h"

namespace {

constexpr int kMaxPositions = 64 * 64 + 1;  // resolution up to 64

__device__ __forceinline__ void edge_point(int xs, int ys, int xe, int ye, int d, int* u, int* v) {
  // point number d (0 .. max(dx, dy)) of the edge (xs, ys) -> (xe, ye) in the order rleFrPoly emits them
  const int dx = abs(xe - xs), dy = abs(ys - ye);
  const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
  int a_xs = xs, a_ys = ys, a_xe = xe, a_ye = ye;
  if (flip) { a_xs = xe; a_xe = xs; a_ys = ye; a_ye = ys; }
  if (dx >= dy) {
    const double s = (double)(a_ye - a_ys) / dx;   // dx == 0 only when the edge is a point: d == 0, s unused (0 * inf guarded)
    const int t = flip ? dx - d : d;
    *u = t + a_xs;
    *v = dx == 0 ? a_ys : (int)(a_ys + s * t + .5);
  } else {
    const double s = (double)(a_xe - a_xs) / dy;
    const int t = flip ? dy - d : d;
    *v = t + a_ys;
    *u = (int)(a_xs + s * t + .5);
  }
}

__global__ __launch_bounds__(64) void project_polygons_kernel(
    const float* __restrict__ coords, const int* __restrict__ poly_start, const int* __restrict__ inst_start,
    const long* __restrict__ gt_index, const float* __restrict__ boxes, int P, int img_w, int img_h, int M,
    float* __restrict__ out) {
  __shared__ int toggles[kMaxPositions];
  __shared__ unsigned char acc[kMaxPositions];
  const int p = blockIdx.x;
  const int lane = threadIdx.x;
  const int npos = M * M;
  for (int i = lane; i < npos; i += 64) acc[i] = 0;
  // PolygonInstance.crop: python-float (double) clamps of the float32 box
  const float4 bb = *(const float4*)(boxes + 4 * (long)p);
  double xmin = bb.x, ymin = bb.y, xmax = bb.z, ymax = bb.w;
  xmin = fmin(fmax(xmin, 0.0), (double)(img_w - 1));
  ymin = fmin(fmax(ymin, 0.0), (double)(img_h - 1));
  xmax = fmin(fmax(xmax, 0.0), (double)img_w);
  ymax = fmin(fmax(ymax, 0.0), (double)img_h);
  xmax = fmax(xmax, xmin + 1.0);
  ymax = fmax(ymax, ymin + 1.0);
  const double w = xmax - xmin, h = ymax - ymin;
  // tensor (float32) - python scalar / * python scalar: the scalar is rounded to float32, the operation is float32
  const float fxmin = (float)xmin, fymin = (float)ymin;
  const float rw = (float)((double)M / w), rh = (float)((double)M / h);
  const long g = gt_index[p];
  for (int poly = inst_start[g]; poly < inst_start[g + 1]; ++poly) {
    const int c0 = poly_start[poly];
    const int k = (poly_start[poly + 1] - c0) / 2;   // vertices
    if (k < 3) continue;                              // PolygonInstance.__init__ drops polygons with < 6 numbers
    for (int i = lane; i <= npos; i += 64) toggles[i] = 0;
    __syncthreads();
    for (int j = 0; j < k; ++j) {
      const int jn = j + 1 == k ? 0 : j + 1;
      // crop + resize in float32, then rleFrPoly's scale-by-5 rounding in double
      const float ax = (coords[c0 + 2 * j] - fxmin) * rw, ay = (coords[c0 + 2 * j + 1] - fymin) * rh;
      const float bx = (coords[c0 + 2 * jn] - fxmin) * rw, by = (coords[c0 + 2 * jn + 1] - fymin) * rh;
      const int xs = (int)(5.0 * (double)ax + .5), ys = (int)(5.0 * (double)ay + .5);
      const int xe = (int)(5.0 * (double)bx + .5), ye = (int)(5.0 * (double)by + .5);
      const int steps = max(abs(xe - xs), abs(ye - ys));
      // consecutive points (d - 1, d), d = 1 .. steps; the pair across two edges is the shared vertex twice: no boundary
      for (int d = 1 + lane; d <= steps; d += 64) {
        int u0, v0, u1, v1;
        edge_point(xs, ys, xe, ye, d - 1, &u0, &v0);
        edge_point(xs, ys, xe, ye, d, &u1, &v1);
        if (u1 == u0) continue;
        double xd = (double)(u1 < u0 ? u1 : u1 - 1);
        xd = (xd + .5) / 5.0 - .5;
        if (floor(xd) != xd || xd < 0 || xd > M - 1) continue;
        double yd = (double)(v1 < v0 ? v1 : v0);
        yd = (yd + .5) / 5.0 - .5;
        if (yd < 0) yd = 0; else if (yd > M) yd = M;
        yd = ceil(yd);
        atomicAdd(&toggles[(int)xd * M + (int)yd], 1);
      }
    }
    __syncthreads();
    // prefix parity over the column-major positions, OR-ed into the instance's mask
    int carry = 0;
    for (int base = 0; base < npos; base += 64) {
      const int i = base + lane;
      int v = i < npos ? (toggles[i] & 1) : 0;
      int incl = v;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
      }
      const int par = (carry + incl) & 1;
      if (i < npos && par) acc[i] = 1;
      carry = (carry + __shfl(incl, 63, 64)) & 1;
    }
    __syncthreads();
  }
  __syncthreads();
  // out[p][y][x]; position = x * M + y (column-major, as the RLE counts)
  float* o = out + (long)p * npos;
  for (int i = lane; i < npos; i += 64) {
    const int y = i / M, x = i - y * M;
    o[i] = (float)acc[x * M + y];
  }
}

// ---- whole-image masks: SegmentationMask(mode='poly').convert('mask') (segmentation_mask.py:326-334) at any canvas size ------
// The device twin of ovis_cpu_polygons_to_masks_u8 (csrc/cpu/ovis_cpu.cpp): no crop, no resize, w x h positions instead of
// M x M.  A million positions do not fit the LDS toggle array above, so the toggles live in the caller's workspace as ONE
// BIT per column-major position and polygon:
//   1. toggle : every boundary point xors its bit (global atomic; xor commutes, so the result does not depend on the order);
//   2. parity : the parity of every chunk of kChunkWords words;
//   3. fill   : per chunk, the xor of the earlier chunks' parities is the carry in; inside the chunk a word's bits become their
//               running parity (shift-xor ladder), words and lanes are chained by ballots -- in place;
//   4. expand : out[g][y][x] = OR over the instance's polygons of bit x * h + y (column-major -> row-major): a lane owns a
//               column and 64 rows (three words, funnel-shifted), a wave writes 64 consecutive bytes per row.
// The parity runs over ALL w * h positions, not per column: a point clamped to y = h toggles the next column's first position.
constexpr int kChunkThreads = 256;
constexpr int kChunkWords = 8 * kChunkThreads;  // 65 536 positions per chunk

__global__ __launch_bounds__(256) void polygon_toggle_kernel(const float* __restrict__ coords, const int* __restrict__ poly_start,
                                                            int w, int h, long words_per_poly, unsigned* __restrict__ bits) {
  const int poly = blockIdx.x;
  const int c0 = poly_start[poly];
  const int k = (poly_start[poly + 1] - c0) / 2;   // vertices
  if (k < 3) return;                                // PolygonInstance.__init__ drops polygons with < 6 numbers
  unsigned* b = bits + (long)poly * words_per_poly;
  const long npos = (long)w * h;
  for (int j = blockIdx.y; j < k; j += gridDim.y) {
    const int jn = j + 1 == k ? 0 : j + 1;
    // rleFrPoly's scale-by-5 rounding in double (_mask.pyx hands the float32 coordinates over as doubles: exact)
    const int xs = (int)(5.0 * (double)coords[c0 + 2 * j] + .5), ys = (int)(5.0 * (double)coords[c0 + 2 * j + 1] + .5);
    const int xe = (int)(5.0 * (double)coords[c0 + 2 * jn] + .5), ye = (int)(5.0 * (double)coords[c0 + 2 * jn + 1] + .5);
    const int steps = max(abs(xe - xs), abs(ye - ys));
    for (int d = 1 + (int)threadIdx.x; d <= steps; d += 256) {
      int u0, v0, u1, v1;
      edge_point(xs, ys, xe, ye, d - 1, &u0, &v0);
      edge_point(xs, ys, xe, ye, d, &u1, &v1);
      if (u1 == u0) continue;
      double xd = (double)(u1 < u0 ? u1 : u1 - 1);
      xd = (xd + .5) / 5.0 - .5;
      if (floor(xd) != xd || xd < 0 || xd > w - 1) continue;
      double yd = (double)(v1 < v0 ? v1 : v0);
      yd = (yd + .5) / 5.0 - .5;
      if (yd < 0) yd = 0; else if (yd > h) yd = h;
      yd = ceil(yd);
      const long pos = (long)xd * h + (long)yd;   // <= w * h; position w * h is behind the last pixel
      if (pos < npos) atomicXor(&b[pos >> 5], 1u << (pos & 31));
    }
  }
}

// parity (0 / 1) of `v` xor-ed over the workgroup's kChunkThreads threads
__device__ __forceinline__ unsigned block_parity(unsigned v, unsigned* sh) {
  const unsigned long long m = __ballot(v & 1u);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = (unsigned)__popcll(m) & 1u;
  __syncthreads();
  unsigned r = 0;
#pragma unroll
  for (int i = 0; i < kChunkThreads / 64; ++i) r ^= sh[i];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kChunkThreads) void polygon_chunk_parity_kernel(const unsigned* __restrict__ bits, int chunks,
                                                                            long words_per_poly,
                                                                            unsigned* __restrict__ chunk_parity) {
  __shared__ unsigned sh[kChunkThreads / 64];
  const int c = blockIdx.x, poly = blockIdx.y;
  const uint4* src = (const uint4*)(bits + (long)poly * words_per_poly + (long)c * kChunkWords) + 2 * threadIdx.x;
  const uint4 a = src[0], b = src[1];
  const unsigned x = a.x ^ a.y ^ a.z ^ a.w ^ b.x ^ b.y ^ b.z ^ b.w;
  const unsigned par = block_parity((unsigned)__popc(x), sh);
  if (threadIdx.x == 0) chunk_parity[(long)poly * chunks + c] = par;
}

__global__ __launch_bounds__(kChunkThreads) void polygon_fill_kernel(unsigned* __restrict__ bits, int chunks, long words_per_poly,
                                                                    const unsigned* __restrict__ chunk_parity) {
  __shared__ unsigned sh[kChunkThreads / 64];
  const int c = blockIdx.x, poly = blockIdx.y, tid = threadIdx.x;
  // carry into the chunk: parity of everything in front of it
  unsigned before = 0;
  for (int i = tid; i < c; i += kChunkThreads) before ^= chunk_parity[(long)poly * chunks + i];
  unsigned carry = block_parity(before, sh);
  uint4* dst = (uint4*)(bits + (long)poly * words_per_poly + (long)c * kChunkWords) + 2 * tid;
  const uint4 a = dst[0], b = dst[1];
  unsigned wd[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  unsigned mine = 0;   // parity of the thread's eight words
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    unsigned v = wd[i];   // bit i := parity of bits 0 .. i
    v ^= v << 1;
    v ^= v << 2;
    v ^= v << 4;
    v ^= v << 8;
    v ^= v << 16;
    wd[i] = v;
    mine ^= v >> 31;
  }
  // threads in front of this one: lower lanes of the wave, then the earlier waves
  const unsigned long long m = __ballot(mine & 1u);
  const int lane = tid & 63, wave = tid >> 6;
  if (lane == 0) sh[wave] = (unsigned)__popcll(m) & 1u;
  __syncthreads();
  carry ^= (unsigned)__popcll(m & ((1ull << lane) - 1ull)) & 1u;
#pragma unroll
  for (int i = 0; i < kChunkThreads / 64; ++i) carry ^= i < wave ? sh[i] : 0u;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const unsigned v = wd[i] ^ (0u - carry);
    carry ^= wd[i] >> 31;
    wd[i] = v;
  }
  dst[0] = make_uint4(wd[0], wd[1], wd[2], wd[3]);
  dst[1] = make_uint4(wd[4], wd[5], wd[6], wd[7]);
}

__global__ __launch_bounds__(256) void polygon_expand_kernel(const unsigned* __restrict__ filled, const int* __restrict__ inst_start,
                                                            int num_polygons, int w, int h, long words_per_poly,
                                                            unsigned char* __restrict__ out) {
  const int x = blockIdx.x * 256 + threadIdx.x, y0 = blockIdx.y * 64, g = blockIdx.z;
  if (x >= w) return;
  const int rows = min(64, h - y0);
  const long pos = (long)x * h + y0;
  const long wi = pos >> 5;
  const int sh = (int)(pos & 31);
  unsigned long long m = 0;
  const int q0 = max(inst_start[g], 0), q1 = min(inst_start[g + 1], num_polygons);
  for (int q = q0; q < q1; ++q) {
    const unsigned* b = filled + (long)q * words_per_poly;
    const unsigned long long a0 = b[wi];
    const unsigned long long a1 = wi + 1 < words_per_poly ? b[wi + 1] : 0u;
    const unsigned long long a2 = wi + 2 < words_per_poly ? b[wi + 2] : 0u;
    const unsigned lo = (unsigned)(((a1 << 32) | a0) >> sh), hi = (unsigned)(((a2 << 32) | a1) >> sh);
    m |= ((unsigned long long)hi << 32) | lo;
  }
  unsigned char* o = out + ((long)g * h + y0) * w + x;
  for (int r = 0; r < rows; ++r) o[(long)r * w] = (unsigned char)((m >> r) & 1ull);
}

}  // namespace

extern "C" int ovis_project_polygon_masks_f32(const float* coords, const int32_t* polygon_start,
                                              const int32_t* instance_start, const int64_t* gt_index, const float* boxes,
                                              int num, int image_width, int image_height, int resolution, float* out,
                                              void* stream) {
  if (num < 0 || resolution <= 0 || image_width <= 0 || image_height <= 0) return OVIS_EINVAL;
  if (num == 0) return OVIS_OK;
  if (!polygon_start || !instance_start || !gt_index || !boxes || !out) return OVIS_EINVAL;
  if (resolution > 64) return OVIS_ERANGE;
  if (((uintptr_t)boxes & 15) != 0) return OVIS_EINVAL;
  hipLaunchKernelGGL(project_polygons_kernel, dim3((unsigned)num), dim3(64), 0, (hipStream_t)stream, coords, polygon_start,
                     instance_start, (const long*)gt_index, boxes, num, image_width, image_height, resolution, out);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}

static long polygon_words(int width, int height) {   // bit words per polygon, whole chunks
  const long words = ((long)width * height + 31) / 32;
  return (words + kChunkWords - 1) / kChunkWords * kChunkWords;
}

extern "C" size_t ovis_polygons_to_masks_workspace_bytes(int num_polygons, int width, int height) {
  if (num_polygons <= 0 || width <= 0 || height <= 0) return 0;
  const long words = polygon_words(width, height);
  return (size_t)num_polygons * (size_t)(words + words / kChunkWords) * sizeof(uint32_t);
}

extern "C" int ovis_polygons_to_masks_u8(const float* coords, const int32_t* polygon_start, const int32_t* instance_start,
                                         int num_instances, int num_polygons, int width, int height, void* workspace,
                                         size_t workspace_bytes, uint8_t* out, void* stream) {
  if (num_instances < 0 || num_polygons < 0 || width <= 0 || height <= 0) return OVIS_EINVAL;
  if (num_instances == 0) return OVIS_OK;
  if (!polygon_start || !instance_start || !out || (num_polygons > 0 && !workspace)) return OVIS_EINVAL;
  if ((long)width * height > (1L << 30) || num_polygons > 65535 || num_instances > 65535) return OVIS_ERANGE;
  if (((uintptr_t)workspace & 15) != 0) return OVIS_EINVAL;
  if (workspace_bytes < ovis_polygons_to_masks_workspace_bytes(num_polygons, width, height)) return OVIS_ENOSPC;
  hipStream_t s = (hipStream_t)stream;
  const long words = polygon_words(width, height);
  const int chunks = (int)(words / kChunkWords);
  unsigned* bits = (unsigned*)workspace;
  unsigned* chunk_parity = bits + (long)num_polygons * words;
  if (num_polygons > 0) {
    OVIS_HIP_TRY(hipMemsetAsync(bits, 0, sizeof(uint32_t) * (size_t)num_polygons * (size_t)words, s));
    hipLaunchKernelGGL(polygon_toggle_kernel, dim3((unsigned)num_polygons, 8), dim3(256), 0, s, coords, polygon_start, width,
                       height, words, bits);
    OVIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(polygon_chunk_parity_kernel, dim3((unsigned)chunks, (unsigned)num_polygons), dim3(kChunkThreads), 0, s, bits,
                       chunks, words, chunk_parity);
    OVIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(polygon_fill_kernel, dim3((unsigned)chunks, (unsigned)num_polygons), dim3(kChunkThreads), 0, s, bits, chunks,
                       words, chunk_parity);
    OVIS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(polygon_expand_kernel, dim3((unsigned)((width + 255) / 256), (unsigned)((height + 63) / 64), (unsigned)num_instances),
                     dim3(256), 0, s, bits, instance_start, num_polygons, width, height, words, (unsigned char*)out);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}
