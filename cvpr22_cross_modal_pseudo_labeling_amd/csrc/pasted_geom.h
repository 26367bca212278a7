// Geometry and per-pixel arithmetic of the Masker paste (mask_head/inference.py:100-160 with padding 1), shared by the
// kernels that evaluate pasted masks: project_pasted_masks_kernel (csrc/targets.hip: the pixels a crop + resize reads) and
// paste_masks_kernel (csrc/paste.hip: every pixel of the canvas).  Both evaluate these expressions, in this order (FP
// contraction is off for the library), so a pixel has the same value whichever kernel asks for it.
#pragma once
#include <hip/hip_runtime.h>

// The integer box a mask is pasted into: the box expanded by (M+2)/M about its centre, truncated toward zero
// (inference.py:69-86 expand_boxes, :114 box.to(torch.int32)); extents max(.., 1) (:118-119).
struct PastedBox {
  int4 bx;     // x0, y0, x1, y1 (inclusive)
  int bw, bh;  // size the padded map is resized to
};

__device__ __forceinline__ PastedBox pasted_box(const float4 gb, int M) {
  const float scale = (float)(M + 2) / (float)M;
  const float w_half = (gb.z - gb.x) * 0.5f * scale, h_half = (gb.w - gb.y) * 0.5f * scale;
  const float x_c = (gb.z + gb.x) * 0.5f, y_c = (gb.w + gb.y) * 0.5f;
  PastedBox b;
  b.bx = make_int4((int)(x_c - w_half), (int)(y_c - h_half), (int)(x_c + w_half), (int)(y_c + h_half));
  b.bw = max(b.bx.z - b.bx.x + 1, 1);
  b.bh = max(b.bx.w - b.bx.y + 1, 1);
  return b;
}

// Pixel (Y, X) INSIDE the integer box and the image: the (M+2)^2 zero-padded map resized bilinearly (align_corners=False)
// to bw x bh, thresholded.  `at(y, x)` reads the padded map, 0 <= y, x <= M + 1.
template <typename At>
__device__ __forceinline__ bool pasted_inside(At&& at, int M, int4 bx, int bw, int bh, float thr, int Y, int X) {
  const int S = M + 2;
  // upsample_bilinear2d, align_corners=False: src = scale * (dst + 0.5) - 0.5 clamped at 0, scale = in / out
  const float scale_y = (float)S / (float)bh, scale_x = (float)S / (float)bw;
  const float sy = fmaxf(scale_y * ((float)(Y - bx.y) + 0.5f) - 0.5f, 0.f);
  const float sx = fmaxf(scale_x * ((float)(X - bx.x) + 0.5f) - 0.5f, 0.f);
  const int y0 = (int)sy, x0 = (int)sx;
  const int y1 = y0 + (y0 < S - 1), x1 = x0 + (x0 < S - 1);
  const float ly = sy - (float)y0, lx = sx - (float)x0;
  const float v = (1.f - ly) * ((1.f - lx) * at(y0, x0) + lx * at(y0, x1)) + ly * ((1.f - lx) * at(y1, x0) + lx * at(y1, x1));
  return v > thr;
}

// Pixel (Y, X) of the binary image mask Masker would paste, from the unpadded M x M map in memory: zero outside the
// image and outside the integer box.
__device__ __forceinline__ float pasted_pixel(const float* __restrict__ prob, int M, int4 bx, int bw, int bh, float thr,
                                              int im_h, int im_w, int Y, int X) {
  if (Y < 0 || X < 0 || Y >= im_h || X >= im_w || Y < bx.y || Y > bx.w || X < bx.x || X > bx.z) return 0.f;
  auto at = [&](int y, int x) {  // the padded map: a zero border of one pixel
    return (y >= 1 && y <= M && x >= 1 && x <= M) ? prob[(y - 1) * M + (x - 1)] : 0.f;
  };
  return pasted_inside(at, M, bx, bw, bh, thr, Y, X) ? 1.f : 0.f;
}
