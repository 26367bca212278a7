// The prediction compositor: box outlines, filled instance masks and uncertainty heat layers blended onto a uint8 HWC image
// in ONE launch (mb/engine/inference.py:519-589: overlay_boxes, overlay_filled_mask, overlay_uncertainty_mask over the
// Masker paste of mask_head/inference.py:124-165).  The reference pastes every instance into a full-size canvas and then
// makes three np.where passes over the whole image per instance; going through ovis_paste_masks_u8 would still
// materialise [K, H, W] masks (31 MB for 100 detections at 480 x 640) and read them back K times.  Here no mask is built:
// every output byte is written once, and a pixel evaluates only the layers whose integer pasted box covers it, in index
// order, truncating to uint8 after each -- the sequential assignment into a uint8 array.
//
// A workgroup owns a kTileW x kTileH tile of pixels; a lane keeps kLanePixels consecutive pixels of one row (12 bytes) in
// registers from the load of the image to the single store.  Wave 0 tests kListCap layers per round against the tile (the
// outline's outer rectangle, then the clipped integer pasted box) and compacts the hits IN ORDER into LDS with a ballot and
// a popcount of the lower lanes; the list is worked off before the next round, so any number of layers may cover a tile.
// For a listed layer the zero-padded (M+2)^2 map is staged in LDS once (as csrc/paste.hip does) and every lane samples it
// through pasted_value() -- the expression sequence the thresholded paste kernels decide with.  All LDS is dynamic (the map,
// then the list): no static variable shifts its base.  No atomics, no workspace, no host read.
//
// Rows start at byte y * W * 3, in general not a multiple of 4: a lane whose 12 bytes are all inside the image and start on
// a 4-byte address moves them as three dwords, every other lane (row tails, odd offsets) byte by byte; nothing outside
// H * W * 3 is touched.
#include "ovis_common.h"
#define OVIS_HD __device__ __forceinline__
#include "pasted_geom.h"
#include "render_geom.h"

namespace {

constexpr int kRenderThreads = 256;
constexpr int kLanePixels = 4;                       // consecutive pixels of a row per lane
constexpr int kLanesX = 16;                          // lanes across a tile row
constexpr int kTileW = kLanesX * kLanePixels;        // 64
constexpr int kTileH = kRenderThreads / kLanesX;     // 16
constexpr int kListCap = 64;                         // layers tested per round: one per lane of wave 0
constexpr int kEntryInts = 12;
constexpr int kRenderMaxM = 120;                     // (M + 2)^2 floats + the list <= 64 KB of LDS

__host__ __device__ constexpr int padded_floats(int M) { return ((M + 2) * (M + 2) + 3) & ~3; }
constexpr int kListInts = kListCap * kEntryInts + 4;  // + the entry count

__global__ __launch_bounds__(kRenderThreads) void render_instances_kernel(
    const unsigned char* __restrict__ image, int H, int W, const float* __restrict__ maps, const float* __restrict__ boxes,
    int K, int M, const int* __restrict__ kinds, const float* __restrict__ params, const float* __restrict__ colors,
    double alpha, const unsigned char* __restrict__ outline_colors, int ol_lo, int ol_hi, unsigned char* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int S = M + 2;
  float* padded = smem;                              // [(M+2), (M+2)]: the map inside a zero border of one pixel
  int* list = (int*)(smem + padded_floats(M));       // [kListCap][kEntryInts], then the count
  int* count = list + kListCap * kEntryInts;

  const int tid = threadIdx.x, lane = tid & 63;
  const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
  const int tx1 = min(tx0 + kTileW, W) - 1, ty1 = min(ty0 + kTileH, H) - 1;  // the tile inside the image (inclusive)
  const int Y = ty0 + (tid / kLanesX), X0 = tx0 + (tid % kLanesX) * kLanePixels;
  const int n = Y < H ? max(min(W - X0, kLanePixels), 0) : 0;                 // this lane's pixels inside the image
  const long off = ((long)Y * W + X0) * 3;

  int px[kLanePixels][3];
#pragma unroll
  for (int j = 0; j < kLanePixels; ++j) px[j][0] = px[j][1] = px[j][2] = 0;
  if (n == kLanePixels && (((uintptr_t)image + off) & 3) == 0) {
    const unsigned* src = (const unsigned*)(image + off);
    const unsigned w0 = src[0], w1 = src[1], w2 = src[2];
    const unsigned w[3] = {w0, w1, w2};
#pragma unroll
    for (int b = 0; b < 3 * kLanePixels; ++b) px[b / 3][b % 3] = (int)((w[b >> 2] >> (8 * (b & 3))) & 255u);
  } else {
#pragma unroll
    for (int j = 0; j < kLanePixels; ++j)
      if (j < n) {
        px[j][0] = image[off + 3 * j];
        px[j][1] = image[off + 3 * j + 1];
        px[j][2] = image[off + 3 * j + 2];
      }
  }

  // ---- outlines: all of them before any layer (visualization_mask draws the boxes first), later boxes over earlier ones
  if (outline_colors != nullptr) {
    for (int base = 0; base < K; base += kListCap) {
      if (tid < 64) {
        const int i = base + lane;
        bool hit = false;
        OutlineRect r{0, 0, 0, 0};
        if (i < K) {
          const float4 gb = *(const float4*)(boxes + 4 * (long)i);
          r = outline_rect(gb.x, gb.y, gb.z, gb.w);
          hit = render_box_sane(gb.x, gb.y, gb.z, gb.w) && r.xa - ol_lo <= tx1 && r.xb + ol_hi >= tx0 &&
                r.ya - ol_lo <= ty1 && r.yb + ol_hi >= ty0;
        }
        const unsigned long long hits = __ballot(hit);
        if (hit) {
          int* e = list + kEntryInts * __popcll(hits & ((1ull << lane) - 1ull));
          e[0] = r.xa;
          e[1] = r.ya;
          e[2] = r.xb;
          e[3] = r.yb;
          e[4] = i;
        }
        if (lane == 0) *count = __popcll(hits);
      }
      __syncthreads();
      const int listed = *count;
      for (int k = 0; k < listed; ++k) {
        const int* e = list + kEntryInts * k;
        const OutlineRect r{e[0], e[1], e[2], e[3]};
        const unsigned char* oc = outline_colors + 3 * (long)e[4];
        const int c0 = oc[0], c1 = oc[1], c2 = oc[2];
#pragma unroll
        for (int j = 0; j < kLanePixels; ++j)
          if (j < n && outline_covers(r, ol_lo, ol_hi, Y, X0 + j)) {
            px[j][0] = c0;
            px[j][1] = c1;
            px[j][2] = c2;
          }
      }
      __syncthreads();  // the list is rewritten by the next round
    }
  }

  // ---- layers, in index order
  auto at = [&](int y, int x) { return padded[y * S + x]; };
  for (int base = 0; base < K; base += kListCap) {
    if (tid < 64) {
      const int i = base + lane;
      bool hit = false;
      PastedBox pb;
      int cx0 = 0, cy0 = 0, cx1 = -1, cy1 = -1, kind = -1;
      if (i < K) {
        const float4 gb = *(const float4*)(boxes + 4 * (long)i);
        pb = pasted_box(gb, M);
        // the box clipped to the image (inclusive; empty when c?1 < c?0)
        cx0 = max(pb.bx.x, 0), cx1 = min(pb.bx.z, W - 1), cy0 = max(pb.bx.y, 0), cy1 = min(pb.bx.w, H - 1);
        kind = kinds[i];
        hit = render_box_sane(gb.x, gb.y, gb.z, gb.w) && (kind == kRenderFill || kind == kRenderHeat) && cx0 <= tx1 &&
              cx1 >= tx0 && cy0 <= ty1 && cy1 >= ty0;
      }
      const unsigned long long hits = __ballot(hit);
      if (hit) {
        int* e = list + kEntryInts * __popcll(hits & ((1ull << lane) - 1ull));
        e[0] = pb.bx.x;
        e[1] = pb.bx.y;
        e[2] = pb.bw;
        e[3] = pb.bh;
        e[4] = cx0;
        e[5] = cy0;
        e[6] = cx1;
        e[7] = cy1;
        e[8] = i;
        e[9] = kind;
        e[10] = __float_as_int(params[i]);
      }
      if (lane == 0) *count = __popcll(hits);
    }
    __syncthreads();
    const int listed = *count;
    __syncthreads();  // an empty list has no barrier below: wave 0 must not start the next round before every wave has read
    for (int k = 0; k < listed; ++k) {
      const int* e = list + kEntryInts * k;
      const int bx0 = e[0], by0 = e[1], bw = e[2], bh = e[3], cx0 = e[4], cy0 = e[5], cx1 = e[6], cy1 = e[7];
      const int i = e[8], kind = e[9];
      const float param = __int_as_float(e[10]);
      const float* pr = maps + (long)i * M * M;
      for (int q = tid; q < S * S; q += kRenderThreads) {
        const int y = q / S, x = q - y * S;
        padded[q] = (y >= 1 && y <= M && x >= 1 && x <= M) ? pr[(y - 1) * M + (x - 1)] : 0.f;
      }
      __syncthreads();
      if (Y >= cy0 && Y <= cy1 && X0 <= cx1 && X0 + kLanePixels - 1 >= cx0) {
        const float col0 = colors[3 * (long)i], col1 = colors[3 * (long)i + 1], col2 = colors[3 * (long)i + 2];
#pragma unroll
        for (int j = 0; j < kLanePixels; ++j) {
          const int X = X0 + j;
          if (X < cx0 || X > cx1) continue;
          const float v = pasted_value(at, M, bx0, by0, bw, bh, Y, X);
          if (kind == kRenderFill) {
            if (v > param) {
              px[j][0] = render_fill(px[j][0], col0, alpha);
              px[j][1] = render_fill(px[j][1], col1, alpha);
              px[j][2] = render_fill(px[j][2], col2, alpha);
            }
          } else {
            const float m = render_heat_weight(v, param);
            if (m != 0.f) {
              px[j][0] = render_heat(px[j][0], m, col0);
              px[j][1] = render_heat(px[j][1], m, col1);
              px[j][2] = render_heat(px[j][2], m, col2);
            }
          }
        }
      }
      __syncthreads();  // the map (and, after the last entry, the list) is rewritten next
    }
  }

  if (n == kLanePixels && (((uintptr_t)out + off) & 3) == 0) {
    unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
    for (int b = 0; b < 3 * kLanePixels; ++b) w[b >> 2] |= ((unsigned)px[b / 3][b % 3] & 255u) << (8 * (b & 3));
    unsigned* dst = (unsigned*)(out + off);
    dst[0] = w[0];
    dst[1] = w[1];
    dst[2] = w[2];
  } else {
#pragma unroll
    for (int j = 0; j < kLanePixels; ++j)
      if (j < n) {
        out[off + 3 * j] = (unsigned char)px[j][0];
        out[off + 3 * j + 1] = (unsigned char)px[j][1];
        out[off + 3 * j + 2] = (unsigned char)px[j][2];
      }
  }
}

}  // namespace

extern "C" int ovis_render_instances_u8(const uint8_t* image, int height, int width, const float* maps, const float* boxes,
                                        int num_layers, int map_resolution, const int32_t* kinds, const float* params,
                                        const float* colors, float alpha, const uint8_t* outline_colors,
                                        int outline_thickness, uint8_t* out, void* stream) {
  if (height <= 0 || width <= 0 || num_layers < 0 || !image || !out || !(alpha >= 0.f && alpha <= 1.f)) return OVIS_EINVAL;
  if (num_layers > 0 && (map_resolution <= 0 || !maps || !boxes || !kinds || !params || !colors)) return OVIS_EINVAL;
  if (num_layers > 0 && outline_colors && outline_thickness < 1) return OVIS_EINVAL;
  if (height > kRenderMaxDim || width > kRenderMaxDim) return OVIS_ERANGE;
  const long bytes = 3L * height * width;
  if ((uintptr_t)image < (uintptr_t)out + bytes && (uintptr_t)out < (uintptr_t)image + bytes) return OVIS_EINVAL;  // aliased
  if (num_layers > 0 && (((uintptr_t)boxes & 15) || map_resolution > kRenderMaxM)) return OVIS_ERANGE;
  if (num_layers > 0 && outline_colors && outline_thickness > kRenderMaxThickness) return OVIS_ERANGE;
  const int M = num_layers > 0 ? map_resolution : 1;
  const int t = outline_thickness;
  const dim3 grid((unsigned)((width + kTileW - 1) / kTileW), (unsigned)((height + kTileH - 1) / kTileH));
  hipLaunchKernelGGL(render_instances_kernel, grid, dim3(kRenderThreads), sizeof(float) * (padded_floats(M) + kListInts),
                     (hipStream_t)stream, (const unsigned char*)image, height, width, maps, boxes, num_layers, M,
                     (const int*)kinds, params, colors, (double)alpha, (const unsigned char*)outline_colors, t / 2,
                     (t + 1) / 2 - 1, (unsigned char*)out);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}
