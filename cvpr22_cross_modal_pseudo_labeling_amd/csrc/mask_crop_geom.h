// The crop window and the per-axis resize taps of the binary-mask targets (mask_head/loss.py:11-42 over BinaryMaskList.crop
// and .resize, structures/segmentation_mask.py:117-156), shared by the kernels that evaluate them: project_masks_kernel and
// project_pasted_masks_kernel (csrc/targets.hip) and project_rle_masks_kernel (csrc/rle_targets.hip).  One sequence of fp32
// expressions (FP contraction is off for the library), so a box crops the same window and an output index reads the same
// taps with the same weights whichever kernel asks.  Like every shared header, this one expects the includer to define
// OVIS_HD (the function qualifiers of its compiler) first.
#pragma once
#include <hip/hip_runtime.h>

// BinaryMaskList.crop (segmentation_mask.py:117-136) on a W x H mask: python round() = half to even, the clamps, and a
// window of at least one pixel.  The window is [ymin, ymin + h) x [xmin, xmin + w), integers held in floats.
struct MaskCropWindow {
  float xmin, ymin, w, h;
};

OVIS_HD MaskCropWindow mask_crop_window(const float4 bx, int W, int H) {
  const float b0 = rintf(bx.x), b1 = rintf(bx.y), b2 = rintf(bx.z), b3 = rintf(bx.w);  // python round(): half to even
  const float xmin = fminf(fmaxf(b0, 0.f), (float)(W - 1)), ymin = fminf(fmaxf(b1, 0.f), (float)(H - 1));
  const float xmax = fmaxf(fminf(fmaxf(b2, 0.f), (float)W), xmin + 1.f);
  const float ymax = fmaxf(fminf(fmaxf(b3, 0.f), (float)H), ymin + 1.f);
  MaskCropWindow c;
  c.xmin = xmin;
  c.ymin = ymin;
  c.w = xmax - xmin;
  c.h = ymax - ymin;
  return c;
}

// Output index d of one axis resized n_in -> n_out by F.interpolate(bilinear, align_corners=False): the two source
// positions (inside [0, n_in - 1], integers held in floats) and the weight `lam` of the second.
// scale = in / out as ONE correctly rounded division (area_pixel_compute_scale of F.interpolate; segmentation_mask.py:
// 150-155): a crop whose size is a multiple of n_out must give integer source positions -- zero weight on the second tap --
// which size * (1 / n_out) misses by an ulp (tests/test_step_golden.py: the reference's own step disagreed there)
struct MaskAxisTap {
  float i0, i1, lam;
};

OVIS_HD MaskAxisTap mask_axis_tap(int d, float n_in, float n_out) {
  const float s = fmaxf(((float)d + 0.5f) * (n_in / n_out) - 0.5f, 0.f);
  float i0 = floorf(s);
  MaskAxisTap t;
  t.lam = s - i0;
  i0 = fminf(i0, n_in - 1.f);
  t.i0 = i0;
  t.i1 = fminf(i0 + 1.f, n_in - 1.f);
  return t;
}
