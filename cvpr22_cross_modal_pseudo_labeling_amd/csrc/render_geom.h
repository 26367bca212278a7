// Per-pixel arithmetic of the prediction compositor (mb/engine/inference.py:519-589: overlay_boxes, overlay_filled_mask,
// overlay_uncertainty_mask), shared by the device kernel (csrc/render.hip) and its host twin (csrc/cpu/ovis_cpu.cpp): both
// evaluate these expressions, in this order (FP contraction is off for both libraries), so a byte is the same on either
// side.  The includer defines OVIS_HD (the function qualifiers of its compiler) before including this file.
#pragma once

constexpr int kRenderFill = 0, kRenderHeat = 1;  // the values of `kinds`
constexpr int kRenderMaxDim = 65535;             // image height and width
constexpr int kRenderMaxThickness = 255;

// A box the compositor follows: every coordinate finite and within +-kRenderMaxCoord, so that the integer boxes and the
// float pixel offsets of pasted_value() are exact.  Any other box (NaN, infinite, absurd) has neither outline nor layer.
constexpr float kRenderMaxCoord = 1.0e6f;
OVIS_HD bool render_box_sane(float gx0, float gy0, float gx1, float gy1) {
  return fabsf(gx0) <= kRenderMaxCoord && fabsf(gy0) <= kRenderMaxCoord && fabsf(gx1) <= kRenderMaxCoord &&
         fabsf(gy1) <= kRenderMaxCoord;
}

// overlay_filled_mask (inference.py:564-566): `uint8 * (1 - 0.5) + 0.5 * color` is a float64 expression in NumPy (a
// Python float meets an integer array), assigned back into the uint8 image: truncated.  p in 0..255, color in 0..255.
OVIS_HD int render_fill(int p, float color, double alpha) { return (int)((double)p * (1.0 - alpha) + alpha * (double)color); }

// overlay_uncertainty_mask (inference.py:584): np.clip(mask * (0.2 / s), 0, 1) on the float32 paste; gain = float32(0.2 / s).
OVIS_HD float render_heat_weight(float v, float gain) { return fminf(fmaxf(v * gain, 0.f), 1.f); }

// overlay_uncertainty_mask (inference.py:585-586): `uint8 * (1 - mask) + mask * color` stays float32 in NumPy (an integer
// array meets a float32 array), one rounding per operation, truncated by the assignment.  The caller skips m == 0.
OVIS_HD int render_heat(int p, float m, float color) { return (int)((float)p * (1.f - m) + m * color); }

// overlay_boxes (inference.py:531-538): the rectangle through the box corners truncated toward zero (box.to(torch.int64)),
// drawn with thickness t.  THE RULE (ours: cv2's coverage of a thick rectangle is not reproduced): the corners are ordered
// (xa <= xb, ya <= yb); an edge at integer coordinate c covers c - floor(t/2) ... c + ceil(t/2) - 1 across its direction
// and runs, along its direction, from the low end of the band of the first corner to the high end of the band of the
// second -- the four corners are filled squares.  Clipped to the image by the caller.
struct OutlineRect {
  int xa, ya, xb, yb;
};

OVIS_HD OutlineRect outline_rect(float gx0, float gy0, float gx1, float gy1) {
  const int x0 = (int)gx0, y0 = (int)gy0, x1 = (int)gx1, y1 = (int)gy1;
  OutlineRect r;
  r.xa = x0 < x1 ? x0 : x1;
  r.xb = x0 < x1 ? x1 : x0;
  r.ya = y0 < y1 ? y0 : y1;
  r.yb = y0 < y1 ? y1 : y0;
  return r;
}

// lo = floor(t/2), hi = ceil(t/2) - 1: pixel (Y, X) lies on the outline when it is inside the outer rectangle and in the
// band of at least one edge.
OVIS_HD bool outline_covers(const OutlineRect r, int lo, int hi, int Y, int X) {
  if (X < r.xa - lo || X > r.xb + hi || Y < r.ya - lo || Y > r.yb + hi) return false;
  return X <= r.xa + hi || X >= r.xb - lo || Y <= r.ya + hi || Y >= r.yb - lo;
}
