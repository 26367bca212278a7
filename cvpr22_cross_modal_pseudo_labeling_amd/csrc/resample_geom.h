// Arithmetic of the input transform (mb/data/transforms/transforms.py:27-62 Resize -> PIL Image.resize(BILINEAR), :105-120
// ToTensor + Normalize), shared by the device kernels (csrc/image_transform.hip) and their host twin (csrc/cpu/ovis_cpu.cpp):
// both evaluate these expressions, in this order (FP contraction is off for both libraries), so a pixel has the same bits
// on either side.  The includer defines OVIS_HD (the function qualifiers of its compiler) before including this file.
//
// PIL resamples one axis at a time (libImaging/Resample.c): for output position xx the triangle filter is centred at
// (xx + 0.5) * in / out, its support 1 * max(in / out, 1) input pixels; the taps' weights are computed in double, divided
// by their sum, quantised to (int)(0.5 + w * 2^22), and the 8-bit result is (2^21 + sum u * k) >> 22 clipped to 0..255.
#pragma once

constexpr int kResamplePrecisionBits = 32 - 8 - 2;  // 22
constexpr int kResampleMaxDim = 16384;              // every image, output and canvas dimension

struct ResampleAxis {
  double scale;    // in / out
  double support;  // filter half-width in input pixels
  double ss;       // 1 / max(scale, 1)
};

OVIS_HD ResampleAxis resample_axis(int in_size, int out_size) {
  ResampleAxis a;
  double filterscale = a.scale = (double)((float)in_size - 0.f) / out_size;
  if (filterscale < 1.0) filterscale = 1.0;
  a.support = 1.0 * filterscale;
  a.ss = 1.0 / filterscale;
  return a;
}

OVIS_HD double resample_triangle(double x) {
  if (x < 0.0) x = -x;
  if (x < 1.0) return 1.0 - x;
  return 0.0;
}

// Output position xx of one axis for three interleaved channels: `at(i, c)` reads channel c of input position i,
// 0 <= i < in_size.  The weights are evaluated twice (their sum first) instead of being stored: a tap count has no bound
// short of in_size (a 16384 -> 1 axis reads every pixel).
template <typename At>
OVIS_HD void resample_position(At&& at, const ResampleAxis a, int in_size, int xx, int out[3]) {
  const double center = 0.0 + (xx + 0.5) * a.scale;
  int xmin = (int)(center - a.support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + a.support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += resample_triangle((x + xmin - center + 0.5) * a.ss);
  int s0 = 1 << (kResamplePrecisionBits - 1), s1 = s0, s2 = s0;
  for (int x = 0; x < xmax; ++x) {
    double w = resample_triangle((x + xmin - center + 0.5) * a.ss);
    if (ww != 0.0) w /= ww;
    const int k = (int)(0.5 + w * (1 << kResamplePrecisionBits));  // the triangle's weights are never negative
    s0 += at(x + xmin, 0) * k;
    s1 += at(x + xmin, 1) * k;
    s2 += at(x + xmin, 2) * k;
  }
  const int s[3] = {s0 >> kResamplePrecisionBits, s1 >> kResamplePrecisionBits, s2 >> kResamplePrecisionBits};
  for (int c = 0; c < 3; ++c) out[c] = s[c] < 0 ? 0 : (s[c] > 255 ? 255 : s[c]);
}

// ToTensor + Normalize of output channel c from the RGB bytes of a pixel: to_bgr255 -- `image[[2, 1, 0]] * 255`, and
// float32 (u / 255) * 255 == u for every byte -- else u / 255 in RGB order; then (v - mean[c]) / std[c], a true division.
OVIS_HD float normalized_channel(const int rgb[3], int c, int to_bgr255, const float* mean, const float* std) {
  const float v = to_bgr255 ? (float)rgb[2 - c] : (float)rgb[c] / 255.f;
  return (v - mean[c]) / std[c];
}

// One image of the batch: 7 int32 per image.
struct ImageDesc {
  int offset;        // of its first byte in the packed buffer
  int in_h, in_w;    // RGB HWC uint8, rows back to back
  int out_h, out_w;  // size after Resize
  int flip_h, flip_v;
};
constexpr int kImageDescInts = 7;

// A descriptor the kernels may follow without leaving the buffers they were given.
OVIS_HD bool image_desc_valid(const ImageDesc d, long data_bytes, int max_in_h, int max_in_w, int pad_h, int pad_w) {
  return d.in_h >= 1 && d.in_w >= 1 && d.out_h >= 1 && d.out_w >= 1 && d.in_h <= max_in_h && d.in_w <= max_in_w &&
         d.out_h <= pad_h && d.out_w <= pad_w && d.offset >= 0 && (long)d.offset + 3L * d.in_h * d.in_w <= data_bytes;
}

// The input positions [lo, hi) output position xx of one axis reads: the xmin / xmax of resample_position, the same
// expressions.  Both ends are non-decreasing in xx, so outputs [a, b] read no position outside [lo(a), hi(b)).
OVIS_HD void resample_span(const ResampleAxis a, int in_size, int xx, int* lo, int* hi) {
  const double center = 0.0 + (xx + 0.5) * a.scale;
  int xmin = (int)(center - a.support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + a.support + 0.5);
  if (xmax > in_size) xmax = in_size;
  *lo = xmin;
  *hi = xmax;
}

// One image of a windowed batch (scale jitter + fixed-size crop): 11 int32, an ImageDesc followed by the window
// [win_y, win_y + win_h) x [win_x, win_x + win_w) in the frame of the resized, FLIPPED image.  out_h x out_w is the full
// resized size, which is never materialised.
struct WindowDesc {
  ImageDesc im;
  int win_y, win_x, win_h, win_w;
};
constexpr int kWindowDescInts = 11;

// The window in the frame of the resized image BEFORE the flips: first row / column.
OVIS_HD int window_first_row(const WindowDesc d) { return d.im.flip_v ? d.im.out_h - d.win_y - d.win_h : d.win_y; }
OVIS_HD int window_first_col(const WindowDesc d) { return d.im.flip_h ? d.im.out_w - d.win_x - d.win_w : d.win_x; }

// The input rows [lo, hi) the window's rows read in the vertical pass (the rows themselves when that pass is skipped).  A
// window that shows every row (no crop on this axis: every scale at or below 1) takes every input row without the fp64 spans.
OVIS_HD void window_input_rows(const WindowDesc d, int* lo, int* hi) {
  if (d.win_h == d.im.out_h) {
    *lo = 0;
    *hi = d.im.in_h;
    return;
  }
  const int y0 = window_first_row(d);
  if (d.im.out_h == d.im.in_h) {
    *lo = y0;
    *hi = y0 + d.win_h;
    return;
  }
  const ResampleAxis a = resample_axis(d.im.in_h, d.im.out_h);
  int unused;
  resample_span(a, d.im.in_h, y0, lo, &unused);
  resample_span(a, d.im.in_h, y0 + d.win_h - 1, &unused, hi);
}

// A windowed descriptor the kernels may follow without leaving the buffers they were given: the image inside the byte
// buffer and the bounds, the window inside [0, out_h) x [0, out_w) and no larger than the canvas.
OVIS_HD bool window_desc_valid(const WindowDesc d, long data_bytes, int max_in_h, int max_in_w, int pad_h, int pad_w) {
  return d.im.in_h >= 1 && d.im.in_w >= 1 && d.im.out_h >= 1 && d.im.out_w >= 1 && d.im.in_h <= max_in_h &&
         d.im.in_w <= max_in_w && d.im.out_h <= kResampleMaxDim && d.im.out_w <= kResampleMaxDim && d.win_y >= 0 &&
         d.win_x >= 0 && d.win_h >= 1 && d.win_w >= 1 && d.win_h <= d.im.out_h - d.win_y && d.win_w <= d.im.out_w - d.win_x &&
         d.win_h <= pad_h && d.win_w <= pad_w && d.im.offset >= 0 &&
         (long)d.im.offset + 3L * d.im.in_h * d.im.in_w <= data_bytes;
}
