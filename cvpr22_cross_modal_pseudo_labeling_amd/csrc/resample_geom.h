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
