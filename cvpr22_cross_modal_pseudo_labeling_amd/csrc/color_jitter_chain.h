// Arithmetic of the colour jitter (mb/data/transforms/transforms.py:88-102 ColorJitter = torchvision's, on PIL images:
// ImageEnhance.Brightness / Contrast / Color and the HSV round trip of adjust_hue), shared by the device kernels
// (csrc/color_jitter.hip) and their host twin (csrc/cpu/ovis_cpu.cpp): both evaluate these expressions, in this order, with
// FP contraction off in both libraries (csrc/Makefile; a*b+c fused into one rounding changes bytes), so a pixel has the same
// bits on either side -- and the bytes PIL produces.  include/ovis_hip.h states the rule in full.  The includer defines
// OVIS_HD (the function qualifiers of its compiler) before including this file.
#pragma once

constexpr int kJitterSlots = 4;  // operation codes of one image, in application order
constexpr int kJitterBrightness = 0, kJitterContrast = 1, kJitterSaturation = 2, kJitterHue = 3, kJitterUnused = -1;

// The part of image_desc_valid (resample_geom.h) that keeps a kernel inside the byte buffers: the jitter reads only
// offset, in_h and in_w of a descriptor.
OVIS_HD bool jitter_desc_in_buffer(int offset, int in_h, int in_w, long data_bytes, int max_in_h, int max_in_w) {
  return in_h >= 1 && in_w >= 1 && in_h <= max_in_h && in_w <= max_in_w && offset >= 0 &&
         (long)offset + 3L * in_h * in_w <= data_bytes;
}

// One image's row of the two tables.  n: the number of operations, -1 for a malformed row (a code outside -1..3, a repeated
// code, a code behind an unused slot) -- such an image is copied unchanged.  contrast: the slot that holds contrast, or n.
struct JitterChain {
  int n, contrast;
  int op[kJitterSlots];
  float param[kJitterSlots];
};

OVIS_HD JitterChain jitter_chain(const int* ops, const float* params) {
  JitterChain c;
  c.n = 0;
  unsigned seen = 0;
  bool ended = false, bad = false;
  for (int i = 0; i < kJitterSlots; ++i) {
    const int o = ops[i];
    c.op[i] = o;
    c.param[i] = params[i];
    if (o == kJitterUnused) {
      ended = true;
    } else if (o < 0 || o > kJitterHue || ended || ((seen >> o) & 1u)) {
      bad = true;
    } else {
      seen |= 1u << o;
      c.n = i + 1;
    }
  }
  if (bad) c.n = -1;
  c.contrast = c.n;
  for (int i = 0; i < kJitterSlots; ++i)
    if (i < c.n && c.op[i] == kJitterContrast) c.contrast = i;
  return c;
}

// ImageEnhance's Image.blend(degenerate, image, factor) for one channel (libImaging/Blend.c): three float32 operations,
// truncation inside [0, 1], clipping outside.  A factor that is not finite cannot leave 0..255 either (NaN -> 0).
OVIS_HD int jitter_blend(int d, int x, float a) {
  const float diff = (float)x - (float)d;
  const float prod = a * diff;
  const float t = (float)d + prod;
  if (a >= 0.f && a <= 1.f) return (int)t;  // between d and x
  if (!(t > 0.f)) return 0;
  if (t >= 255.f) return 255;
  return (int)t;
}

// convert("L") of one pixel (libImaging/Convert.c: L24 >> 16 with the half added)
OVIS_HD int jitter_grey(const int rgb[3]) { return (rgb[0] * 19595 + rgb[1] * 38470 + rgb[2] * 7471 + 0x8000) >> 16; }

// ImageEnhance.Contrast's degenerate value: int(ImageStat mean of convert("L") + 0.5), the division and the sum in fp64
OVIS_HD int jitter_contrast_mean(long grey_sum, long pixels) { return (int)((double)grey_sum / (double)pixels + 0.5); }

OVIS_HD int jitter_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// convert("HSV") of one pixel (Convert.c rgb2hsv_row).  Where float32 ends and double begins is part of the result.
OVIS_HD void jitter_rgb_to_hsv(const int rgb[3], int hsv[3]) {
  const int r = rgb[0], g = rgb[1], b = rgb[2];
  const int maxc = r > g ? (r > b ? r : b) : (g > b ? g : b), minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
  hsv[2] = maxc;
  if (maxc == minc) {
    hsv[0] = hsv[1] = 0;
    return;
  }
  const float cr = (float)(maxc - minc);
  const float sat = cr / (float)maxc;
  const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
  float hf;
  if (r == maxc) {
    hf = bc - gc;
  } else if (g == maxc) {
    hf = (float)(2.0 + (double)rc - (double)bc);
  } else {
    hf = (float)(4.0 + (double)gc - (double)rc);
  }
  // fmod(hf / 6.0 + 1.0, 1.0): the argument lies in [5/6, 11/6], where the remainder is this exact subtraction
  double turn = (double)hf / 6.0 + 1.0;
  if (turn >= 1.0) turn = turn - 1.0;
  hf = (float)turn;
  hsv[0] = jitter_clip8((int)((double)hf * 255.0));
  hsv[1] = jitter_clip8((int)(sat * 255.f));
}

OVIS_HD int jitter_round8(double x) { return jitter_clip8((int)floor(x + 0.5)); }

// convert("RGB") of one HSV pixel (Convert.c hsv2rgb), in fp64
OVIS_HD void jitter_hsv_to_rgb(const int hsv[3], int rgb[3]) {
  const int h = hsv[0], s = hsv[1], v = hsv[2];
  if (s == 0) {
    rgb[0] = rgb[1] = rgb[2] = v;
    return;
  }
  const double hh = h * 6.0 / 255.0;
  const double fl = floor(hh);
  const double f = hh - fl, fs = s / 255.0;
  const int p = jitter_round8(v * (1.0 - fs)), q = jitter_round8(v * (1.0 - fs * f)),
            t = jitter_round8(v * (1.0 - fs * (1.0 - f)));
  int r, g, b;
  switch ((int)fl % 6) {
    case 0: r = v, g = t, b = p; break;
    case 1: r = q, g = v, b = p; break;
    case 2: r = p, g = v, b = t; break;
    case 3: r = p, g = q, b = v; break;
    case 4: r = t, g = p, b = v; break;
    default: r = v, g = p, b = q; break;
  }
  rgb[0] = r, rgb[1] = g, rgb[2] = b;
}

// One operation on one pixel.  `mean` is the contrast operation's degenerate value.
OVIS_HD void jitter_step(int op, float a, int mean, int rgb[3]) {
  if (op == kJitterBrightness) {
    for (int k = 0; k < 3; ++k) rgb[k] = jitter_blend(0, rgb[k], a);
  } else if (op == kJitterContrast) {
    for (int k = 0; k < 3; ++k) rgb[k] = jitter_blend(mean, rgb[k], a);
  } else if (op == kJitterSaturation) {
    const int grey = jitter_grey(rgb);
    for (int k = 0; k < 3; ++k) rgb[k] = jitter_blend(grey, rgb[k], a);
  } else {  // the shift is an integer 0..255 held exactly; anything else in the table shifts by 0
    const int shift = (a >= 0.f && a <= 255.f) ? (int)a : 0;
    int hsv[3];
    jitter_rgb_to_hsv(rgb, hsv);
    hsv[0] = (hsv[0] + shift) & 255;
    jitter_hsv_to_rgb(hsv, rgb);
  }
}

// Operations [0, last) of a chain on one pixel, each on the previous one's 8-bit result; `mean`: the grey mean of the image
// as the operations in front of contrast left it.  Written out per slot: the tables are indexed by constants only.
OVIS_HD void jitter_apply(const JitterChain& c, int last, int mean, int rgb[3]) {
  if (last > 0) jitter_step(c.op[0], c.param[0], mean, rgb);
  if (last > 1) jitter_step(c.op[1], c.param[1], mean, rgb);
  if (last > 2) jitter_step(c.op[2], c.param[2], mean, rgb);
  if (last > 3) jitter_step(c.op[3], c.param[3], mean, rgb);
}
