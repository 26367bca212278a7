// Geometry and per-pixel arithmetic of the Masker paste (mask_head/inference.py:100-160 with padding 1), shared by the
// kernels that evaluate pasted masks: project_pasted_masks_kernel (csrc/targets.hip: the pixels a crop + resize reads) and
// paste_masks_kernel (csrc/paste.hip: every pixel of the canvas).  Both evaluate the expressions of pasted_value.h, in
// their order (FP contraction is off for the library), so a pixel has the same value whichever kernel asks for it; the
// `> threshold` decision here and the value csrc/render.hip blends with are that one sequence.  Like every shared header,
// this one expects the includer to define OVIS_HD (the function qualifiers of its compiler) first.
#pragma once
#include <hip/hip_runtime.h>

#include "pasted_value.h"  // the includer has defined OVIS_HD

// The integer box a mask is pasted into: the box expanded by (M+2)/M about its centre, truncated toward zero
// (inference.py:69-86 expand_boxes, :114 box.to(torch.int32)); extents max(.., 1) (:118-119).
struct PastedBox {
  int4 bx;     // x0, y0, x1, y1 (inclusive)
  int bw, bh;  // size the padded map is resized to
};

__device__ __forceinline__ PastedBox pasted_box(const float4 gb, int M) {
  const PastedRect r = pasted_rect(gb.x, gb.y, gb.z, gb.w, M);
  PastedBox b;
  b.bx = make_int4(r.x0, r.y0, r.x1, r.y1);
  b.bw = r.bw;
  b.bh = r.bh;
  return b;
}

// Pixel (Y, X) INSIDE the integer box and the image: the (M+2)^2 zero-padded map resized bilinearly (align_corners=False)
// to bw x bh, thresholded.  `at(y, x)` reads the padded map, 0 <= y, x <= M + 1.
template <typename At>
__device__ __forceinline__ bool pasted_inside(At&& at, int M, int4 bx, int bw, int bh, float thr, int Y, int X) {
  return pasted_value(at, M, bx.x, bx.y, bw, bh, Y, X) > thr;
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
