// The Masker paste as plain arithmetic (mask_head/inference.py:96-165 with padding 1): the integer box a map is pasted
// into and the bilinear value of one pixel inside it.  ONE expression sequence, evaluated by every kernel that needs a
// pasted pixel -- the thresholded masks (pasted_geom.h: csrc/paste.hip, csrc/targets.hip), the un-thresholded value of the
// compositor (csrc/render.hip) -- and by the compositor's host twin (csrc/cpu/ovis_cpu.cpp).  FP contraction is off for
// both libraries, so a pixel has the same bits whoever asks for it.  The includer defines OVIS_HD (the function qualifiers
// of its compiler) before including this file.
#pragma once

// The box expanded by (M+2)/M about its centre, truncated toward zero (inference.py:96-110 expand_boxes, :132
// box.to(torch.int32)); extents max(.., 1) (:135-138).
struct PastedRect {
  int x0, y0, x1, y1;  // inclusive
  int bw, bh;          // size the padded map is resized to
};

OVIS_HD PastedRect pasted_rect(float gx0, float gy0, float gx1, float gy1, int M) {
  const float scale = (float)(M + 2) / (float)M;
  const float w_half = (gx1 - gx0) * 0.5f * scale, h_half = (gy1 - gy0) * 0.5f * scale;
  const float x_c = (gx1 + gx0) * 0.5f, y_c = (gy1 + gy0) * 0.5f;
  PastedRect r;
  r.x0 = (int)(x_c - w_half);
  r.y0 = (int)(y_c - h_half);
  r.x1 = (int)(x_c + w_half);
  r.y1 = (int)(y_c + h_half);
  r.bw = r.x1 - r.x0 + 1 > 1 ? r.x1 - r.x0 + 1 : 1;
  r.bh = r.y1 - r.y0 + 1 > 1 ? r.y1 - r.y0 + 1 : 1;
  return r;
}

// Pixel (Y, X) INSIDE the integer box whose corner is (bx0, by0): the (M+2)^2 zero-padded map resized bilinearly
// (align_corners=False) to bw x bh.  `at(y, x)` reads the padded map, 0 <= y, x <= M + 1.
template <typename At>
OVIS_HD float pasted_value(At&& at, int M, int bx0, int by0, int bw, int bh, int Y, int X) {
  const int S = M + 2;
  // upsample_bilinear2d, align_corners=False: src = scale * (dst + 0.5) - 0.5 clamped at 0, scale = in / out
  const float scale_y = (float)S / (float)bh, scale_x = (float)S / (float)bw;
  const float sy = fmaxf(scale_y * ((float)(Y - by0) + 0.5f) - 0.5f, 0.f);
  const float sx = fmaxf(scale_x * ((float)(X - bx0) + 0.5f) - 0.5f, 0.f);
  const int y0 = (int)sy, x0 = (int)sx;
  const int y1 = y0 + (y0 < S - 1), x1 = x0 + (x0 < S - 1);
  const float ly = sy - (float)y0, lx = sx - (float)x0;
  return (1.f - ly) * ((1.f - lx) * at(y0, x0) + lx * at(y0, x1)) + ly * ((1.f - lx) * at(y1, x0) + lx * at(y1, x1));
}
