// libovis_cpu.so: host twins of the two native ops the reference implements on the CPU (RoIAlign forward, NMS) plus the
// RoIAlign transpose -- see include/ovis_cpu.h for the contract and the reference lines.  Product code for HOST tensors of the
// reference's CPU-only configuration; device tensors never come here.
//
// RoIAlign is evaluated SEPARABLY: the sampling positions of a RoI along y and along x do not depend on each other
// (the reference's joint table of pooled_h * pooled_w * grid_h * grid_w entries is the outer product of two short per-axis
// tables), so a RoI builds pooled_h * grid_h + pooled_w * grid_w axis samples once and every channel re-uses them.  The
// floating-point expressions per output are the reference's, in its order.
#include "ovis_cpu.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#ifdef _OPENMP
#include <omp.h>
#endif

#define OVIS_HD static inline
#include "../color_jitter_chain.h"
#include "../pasted_value.h"
#include "../render_geom.h"
#include "../resample_geom.h"

namespace {

struct AxisSample {  // one sampling coordinate along one axis
  int lo, hi;        // the two cells it interpolates between
  float frac, rest;  // frac = distance from cell lo (the weight of cell hi), rest = 1 - frac (the weight of cell lo)
  bool inside;       // false: the coordinate lies outside [-1, size] and contributes nothing
};

AxisSample axis_sample(float v, int size) {
  AxisSample s{0, 0, 0.f, 0.f, false};
  if (v < -1.0f || v > (float)size) return s;
  if (v <= 0.f) v = 0.f;
  s.lo = (int)v;
  if (s.lo >= size - 1) {
    s.hi = s.lo = size - 1;
    v = (float)s.lo;
  } else {
    s.hi = s.lo + 1;
  }
  s.frac = v - (float)s.lo;
  s.rest = 1.f - s.frac;
  s.inside = true;
  return s;
}

struct RoiGeometry {
  int image;
  int grid_h, grid_w;
  float count;
  std::vector<AxisSample> ys, xs;  // [pooled * grid] per axis, bin-major
};

RoiGeometry roi_geometry(const float* roi, int height, int width, int pooled_h, int pooled_w, float scale, int sampling_ratio) {
  RoiGeometry g;
  g.image = (int)roi[0];
  const float start_w = roi[1] * scale, start_h = roi[2] * scale, end_w = roi[3] * scale, end_h = roi[4] * scale;
  const float roi_w = std::max(end_w - start_w, 1.f), roi_h = std::max(end_h - start_h, 1.f);
  const float bin_h = roi_h / (float)pooled_h, bin_w = roi_w / (float)pooled_w;
  g.grid_h = sampling_ratio > 0 ? sampling_ratio : (int)std::ceil(roi_h / pooled_h);
  g.grid_w = sampling_ratio > 0 ? sampling_ratio : (int)std::ceil(roi_w / pooled_w);
  g.count = (float)(g.grid_h * g.grid_w);
  g.ys.resize((size_t)pooled_h * g.grid_h);
  g.xs.resize((size_t)pooled_w * g.grid_w);
  for (int ph = 0; ph < pooled_h; ++ph)
    for (int iy = 0; iy < g.grid_h; ++iy)
      g.ys[(size_t)ph * g.grid_h + iy] = axis_sample(start_h + ph * bin_h + (float)(iy + .5f) * bin_h / (float)g.grid_h, height);
  for (int pw = 0; pw < pooled_w; ++pw)
    for (int ix = 0; ix < g.grid_w; ++ix)
      g.xs[(size_t)pw * g.grid_w + ix] = axis_sample(start_w + pw * bin_w + (float)(ix + .5f) * bin_w / (float)g.grid_w, width);
  return g;
}

int thread_count(int threads) {
#ifdef _OPENMP
  return threads > 0 ? threads : omp_get_max_threads();
#else
  (void)threads;
  return 1;
#endif
}

}  // namespace

extern "C" int ovis_cpu_roi_align_forward_f32(const float* input, const float* rois, float* out, int num_rois, int batch,
                                              int channels, int height, int width, int pooled_h, int pooled_w,
                                              float spatial_scale, int sampling_ratio, int threads) {
  if (num_rois < 0 || batch < 0 || channels < 0 || height <= 0 || width <= 0 || pooled_h <= 0 || pooled_w <= 0) return OVIS_CPU_EINVAL;
  if (num_rois == 0 || channels == 0) return OVIS_CPU_OK;
  if (!input || !rois || !out) return OVIS_CPU_EINVAL;
  for (int r = 0; r < num_rois; ++r) {
    const int b = (int)rois[(size_t)r * 5];
    if (b < 0 || b >= batch) return OVIS_CPU_EINVAL;
  }
  const size_t plane = (size_t)height * width, bins = (size_t)pooled_h * pooled_w;
  const int nt = thread_count(threads);
#pragma omp parallel for schedule(dynamic, 1) num_threads(nt)
  for (int r = 0; r < num_rois; ++r) {
    const RoiGeometry g = roi_geometry(rois + (size_t)r * 5, height, width, pooled_h, pooled_w, spatial_scale, sampling_ratio);
    for (int c = 0; c < channels; ++c) {
      const float* src = input + ((size_t)g.image * channels + c) * plane;
      float* dst = out + ((size_t)r * channels + c) * bins;
      for (int ph = 0; ph < pooled_h; ++ph) {
        for (int pw = 0; pw < pooled_w; ++pw) {
          float acc = 0.f;
          for (int iy = 0; iy < g.grid_h; ++iy) {
            const AxisSample& y = g.ys[(size_t)ph * g.grid_h + iy];
            if (!y.inside) continue;
            const float* row_lo = src + (size_t)y.lo * width;
            const float* row_hi = src + (size_t)y.hi * width;
            for (int ix = 0; ix < g.grid_w; ++ix) {
              const AxisSample& x = g.xs[(size_t)pw * g.grid_w + ix];
              if (!x.inside) continue;
              const float w1 = y.rest * x.rest, w2 = y.rest * x.frac, w3 = y.frac * x.rest, w4 = y.frac * x.frac;
              acc += w1 * row_lo[x.lo] + w2 * row_lo[x.hi] + w3 * row_hi[x.lo] + w4 * row_hi[x.hi];
            }
          }
          dst[(size_t)ph * pooled_w + pw] = acc / g.count;
        }
      }
    }
  }
  return OVIS_CPU_OK;
}

extern "C" int ovis_cpu_roi_align_backward_f32(const float* grad_out, const float* rois, float* grad_input, int num_rois,
                                               int batch, int channels, int height, int width, int pooled_h, int pooled_w,
                                               float spatial_scale, int sampling_ratio, int threads) {
  if (num_rois < 0 || batch < 0 || channels < 0 || height <= 0 || width <= 0 || pooled_h <= 0 || pooled_w <= 0) return OVIS_CPU_EINVAL;
  const size_t plane = (size_t)height * width, bins = (size_t)pooled_h * pooled_w;
  if ((size_t)batch * channels > 0) {
    if (!grad_input) return OVIS_CPU_EINVAL;
    std::memset(grad_input, 0, sizeof(float) * (size_t)batch * channels * plane);
  }
  if (num_rois == 0 || channels == 0) return OVIS_CPU_OK;
  if (!grad_out || !rois) return OVIS_CPU_EINVAL;
  std::vector<RoiGeometry> geo;
  geo.reserve(num_rois);
  for (int r = 0; r < num_rois; ++r) {
    geo.push_back(roi_geometry(rois + (size_t)r * 5, height, width, pooled_h, pooled_w, spatial_scale, sampling_ratio));
    if (geo.back().image < 0 || geo.back().image >= batch) return OVIS_CPU_EINVAL;
  }
  const int nt = thread_count(threads);
  // a thread owns channel c of every image: no two threads touch the same plane, RoIs are visited in order
#pragma omp parallel for schedule(static) num_threads(nt)
  for (int c = 0; c < channels; ++c) {
    for (int r = 0; r < num_rois; ++r) {
      const RoiGeometry& g = geo[r];
      float* dst = grad_input + ((size_t)g.image * channels + c) * plane;
      const float* src = grad_out + ((size_t)r * channels + c) * bins;
      for (int ph = 0; ph < pooled_h; ++ph) {
        for (int pw = 0; pw < pooled_w; ++pw) {
          const float top = src[(size_t)ph * pooled_w + pw];
          for (int iy = 0; iy < g.grid_h; ++iy) {
            const AxisSample& y = g.ys[(size_t)ph * g.grid_h + iy];
            if (!y.inside) continue;
            float* row_lo = dst + (size_t)y.lo * width;
            float* row_hi = dst + (size_t)y.hi * width;
            for (int ix = 0; ix < g.grid_w; ++ix) {
              const AxisSample& x = g.xs[(size_t)pw * g.grid_w + ix];
              if (!x.inside) continue;
              row_lo[x.lo] += top * (y.rest * x.rest) / g.count;
              row_lo[x.hi] += top * (y.rest * x.frac) / g.count;
              row_hi[x.lo] += top * (y.frac * x.rest) / g.count;
              row_hi[x.hi] += top * (y.frac * x.frac) / g.count;
            }
          }
        }
      }
    }
  }
  return OVIS_CPU_OK;
}

extern "C" int ovis_cpu_nms_f32(const float* boxes, const float* scores, int num_boxes, float threshold, int64_t* keep) {
  if (num_boxes < 0) return OVIS_CPU_EINVAL;
  if (num_boxes == 0) return 0;
  if (!boxes || !scores || !keep) return OVIS_CPU_EINVAL;
  std::vector<int> order(num_boxes);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return scores[a] > scores[b]; });
  std::vector<float> area(num_boxes);
  for (int i = 0; i < num_boxes; ++i) {
    const float* q = boxes + (size_t)i * 4;
    area[i] = (q[2] - q[0] + 1) * (q[3] - q[1] + 1);
  }
  std::vector<char> gone(num_boxes, 0);
  for (int oi = 0; oi < num_boxes; ++oi) {
    const int i = order[oi];
    if (gone[i]) continue;
    const float* a = boxes + (size_t)i * 4;
    for (int oj = oi + 1; oj < num_boxes; ++oj) {
      const int j = order[oj];
      if (gone[j]) continue;
      const float* b = boxes + (size_t)j * 4;
      const float w = std::max(0.f, std::min(a[2], b[2]) - std::max(a[0], b[0]) + 1);
      const float h = std::max(0.f, std::min(a[3], b[3]) - std::max(a[1], b[1]) + 1);
      const float inter = w * h;
      if (inter / (area[i] + area[j] - inter) >= threshold) gone[j] = 1;
    }
  }
  int n = 0;
  for (int i = 0; i < num_boxes; ++i)
    if (!gone[i]) keep[n++] = i;
  return n;
}

// ---- polygon ground truth -> M x M mask targets (mask_head/loss.py:11-42 on SegmentationMask(mode='poly') targets) ------------
// PolygonInstance.crop (segmentation_mask.py:270-296: python-float clamps of the box) -> resize (:298-324: float32 tensor x
// python scalar) -> convert_to_binarymask (:326-334: pycocotools.mask.frPyObjects -> merge -> decode; pycocotools==2.0,
// common/maskApi.c rleFrPoly / rleMerge / rleDecode -- a third-party dependency outside /root/reference, its published
// algorithm followed here as in csrc/polygons.hip).  Host form: one positive at a time, a dense walk of every edge on the
// x5 grid; a boundary point TOGGLES its column-major position and the decoded mask is the running parity of the toggles
// (equal positions cancel, as equal run boundaries do in the RLE) -- no sort, no run lengths.
static inline void edge_point(int xs, int ys, int xe, int ye, int d, int& u, int& v) {
  const int dx = std::abs(xe - xs), dy = std::abs(ys - ye);
  const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
  if (flip) { std::swap(xs, xe); std::swap(ys, ye); }
  if (dx >= dy) {
    const int t = flip ? dx - d : d;
    u = t + xs;
    v = dx == 0 ? ys : (int)(ys + ((double)(ye - ys) / dx) * t + .5);
  } else {
    const int t = flip ? dy - d : d;
    v = t + ys;
    u = (int)(xs + ((double)(xe - xs) / dy) * t + .5);
  }
}

// Walks the closed polygon whose x5-grid vertices are (xs[j], ys[j]) and toggles the column-major position of every boundary point
// (rleFrPoly steps 2-4) on a w x h grid: toggles has w * h + 1 entries.
static void toggle_boundary(const std::vector<int>& xs, const std::vector<int>& ys, int w, int h, std::vector<int>& toggles) {
  const int k = (int)xs.size();
  for (int j = 0; j < k; ++j) {
    const int jn = j + 1 == k ? 0 : j + 1;
    const int steps = std::max(std::abs(xs[jn] - xs[j]), std::abs(ys[jn] - ys[j]));
    int u0, v0;
    edge_point(xs[j], ys[j], xs[jn], ys[jn], 0, u0, v0);
    for (int d = 1; d <= steps; ++d) {
      int u1, v1;
      edge_point(xs[j], ys[j], xs[jn], ys[jn], d, u1, v1);
      if (u1 != u0) {
        const double xd = ((double)(u1 < u0 ? u1 : u1 - 1) + .5) / 5.0 - .5;
        if (std::floor(xd) == xd && xd >= 0 && xd <= w - 1) {
          double yd = ((double)std::min(v1, v0) + .5) / 5.0 - .5;
          yd = std::ceil(yd < 0 ? 0.0 : (yd > h ? (double)h : yd));
          toggles[(size_t)xd * h + (size_t)yd] ^= 1;
        }
      }
      u0 = u1;
      v0 = v1;
    }
  }
}

// Whole-image masks of polygon instances: SegmentationMask(mode='poly').convert('mask') (mb/structures/segmentation_mask.py:326-334:
// frPyObjects -> merge -> decode at the image size, no crop / resize).  out [num_instances, height, width] uint8.
extern "C" int ovis_cpu_polygons_to_masks_u8(const float* coords, const int32_t* polygon_start, const int32_t* instance_start,
                                             int num_instances, int width, int height, uint8_t* out, int threads) {
  if (num_instances < 0 || width <= 0 || height <= 0) return OVIS_CPU_EINVAL;
  if (num_instances == 0) return OVIS_CPU_OK;
  if (!polygon_start || !instance_start || !out) return OVIS_CPU_EINVAL;
  const size_t npos = (size_t)width * height;
#ifdef _OPENMP
  if (threads > 0) omp_set_num_threads(threads);
#pragma omp parallel for schedule(dynamic)
#endif
  for (int g = 0; g < num_instances; ++g) {
    std::vector<int> toggles(npos + 1);
    uint8_t* o = out + (size_t)g * npos;
    std::memset(o, 0, npos);
    for (int poly = instance_start[g]; poly < instance_start[g + 1]; ++poly) {
      const int c0 = polygon_start[poly], k = (polygon_start[poly + 1] - c0) / 2;
      if (k < 3) continue;
      std::fill(toggles.begin(), toggles.end(), 0);
      std::vector<int> xs(k), ys(k);
      for (int j = 0; j < k; ++j) {  // _mask.pyx hands the coordinates over as doubles: float32 -> double is exact
        xs[j] = (int)(5.0 * (double)coords[c0 + 2 * j] + .5);
        ys[j] = (int)(5.0 * (double)coords[c0 + 2 * j + 1] + .5);
      }
      toggle_boundary(xs, ys, width, height, toggles);
      int parity = 0;
      for (int x = 0; x < width; ++x)
        for (int y = 0; y < height; ++y) {
          parity ^= toggles[(size_t)x * height + y];
          if (parity) o[(size_t)y * width + x] = 1;
        }
    }
  }
  return OVIS_CPU_OK;
}

extern "C" int ovis_cpu_project_polygon_masks_f32(const float* coords, const int32_t* polygon_start, const int32_t* instance_start,
                                                  const int64_t* gt_index, const float* boxes, int num, int image_width,
                                                  int image_height, int resolution, float* out, int threads) {
  if (num < 0 || resolution <= 0 || image_width <= 0 || image_height <= 0) return OVIS_CPU_EINVAL;
  if (num == 0) return OVIS_CPU_OK;
  if (!polygon_start || !instance_start || !gt_index || !boxes || !out) return OVIS_CPU_EINVAL;
  const int M = resolution, npos = M * M;
#ifdef _OPENMP
  if (threads > 0) omp_set_num_threads(threads);
#pragma omp parallel for schedule(dynamic)
#endif
  for (int p = 0; p < num; ++p) {
    std::vector<int> toggles(npos + 1);
    std::vector<char> acc(npos, 0);
    double xmin = boxes[4 * (size_t)p], ymin = boxes[4 * (size_t)p + 1], xmax = boxes[4 * (size_t)p + 2], ymax = boxes[4 * (size_t)p + 3];
    xmin = std::min(std::max(xmin, 0.0), (double)(image_width - 1));
    ymin = std::min(std::max(ymin, 0.0), (double)(image_height - 1));
    xmax = std::min(std::max(xmax, 0.0), (double)image_width);
    ymax = std::min(std::max(ymax, 0.0), (double)image_height);
    xmax = std::max(xmax, xmin + 1.0);
    ymax = std::max(ymax, ymin + 1.0);
    const float fxmin = (float)xmin, fymin = (float)ymin;
    const float rw = (float)((double)M / (xmax - xmin)), rh = (float)((double)M / (ymax - ymin));
    const int64_t g = gt_index[p];
    for (int poly = instance_start[g]; poly < instance_start[g + 1]; ++poly) {
      const int c0 = polygon_start[poly], k = (polygon_start[poly + 1] - c0) / 2;
      if (k < 3) continue;  // PolygonInstance.__init__ drops polygons with fewer than 6 numbers
      std::fill(toggles.begin(), toggles.end(), 0);
      std::vector<int> xs(k), ys(k);
      for (int j = 0; j < k; ++j) {  // crop + resize in float32, then rleFrPoly's scale-by-5 rounding in double
        const float ax = (coords[c0 + 2 * j] - fxmin) * rw, ay = (coords[c0 + 2 * j + 1] - fymin) * rh;
        xs[j] = (int)(5.0 * (double)ax + .5);
        ys[j] = (int)(5.0 * (double)ay + .5);
      }
      toggle_boundary(xs, ys, M, M, toggles);
      int parity = 0;
      for (int i = 0; i < npos; ++i) {
        parity ^= toggles[i];
        if (parity) acc[i] = 1;  // union over the instance's polygons (rleMerge, intersect = 0)
      }
    }
    float* o = out + (size_t)p * npos;  // out[p][y][x]; positions are column-major (x * M + y), as the RLE counts
    for (int y = 0; y < M; ++y)
      for (int x = 0; x < M; ++x) o[y * M + x] = (float)acc[x * M + y];
  }
  return OVIS_CPU_OK;
}

// ---- the input transform: host twin of ovis_transform_images_u8 (csrc/image_transform.hip), the arithmetic of resample_geom.h --
extern "C" int ovis_cpu_transform_images_u8(const uint8_t* data, long data_bytes, const int32_t* desc, int batch,
                                            const float* mean, const float* std, int to_bgr255, int pad_h, int pad_w,
                                            float* out, int threads) {
  if (batch < 0 || pad_h <= 0 || pad_w <= 0 || data_bytes < 0) return OVIS_CPU_EINVAL;
  if (batch == 0) return OVIS_CPU_OK;
  if (!data || !desc || !mean || !std || !out) return OVIS_CPU_EINVAL;
  if (pad_h > kResampleMaxDim || pad_w > kResampleMaxDim || batch > 65535) return OVIS_CPU_ERANGE;
  for (int b = 0; b < batch; ++b) {
    const int32_t* d = desc + (long)b * kImageDescInts;
    if (d[1] > kResampleMaxDim || d[2] > kResampleMaxDim) return OVIS_CPU_ERANGE;  // out_h, out_w <= pad_h, pad_w
    if (!image_desc_valid(ImageDesc{d[0], d[1], d[2], d[3], d[4], d[5], d[6]}, data_bytes, kResampleMaxDim, kResampleMaxDim,
                          pad_h, pad_w))
      return OVIS_CPU_EINVAL;
  }
  const long plane = (long)pad_h * pad_w;
  const int nt = thread_count(threads);
  for (int b = 0; b < batch; ++b) {
    const int32_t* dd = desc + (long)b * kImageDescInts;
    const ImageDesc d{dd[0], dd[1], dd[2], dd[3], dd[4], dd[5], dd[6]};
    const uint8_t* src = data + d.offset;
    // horizontal pass -> uint8 [in_h, out_w, 3]; skipped when the width does not change (Resample.c: need_horizontal)
    std::vector<uint8_t> rows;
    long stride = 3L * d.in_w;
    if (d.out_w != d.in_w) {
      rows.resize(3UL * d.in_h * d.out_w);
      stride = 3L * d.out_w;
      const ResampleAxis ax = resample_axis(d.in_w, d.out_w);
#pragma omp parallel for schedule(static) num_threads(nt)
      for (int x = 0; x < d.out_w; ++x) {  // a column's weights are the same in every row; the values do not depend on the order
        for (int y = 0; y < d.in_h; ++y) {
          const uint8_t* row = src + 3L * y * d.in_w;
          int u[3];
          resample_position([&](int i, int c) { return (int)row[3 * i + c]; }, ax, d.in_w, x, u);
          for (int c = 0; c < 3; ++c) rows[y * stride + 3L * x + c] = (uint8_t)u[c];
        }
      }
      src = rows.data();
    }
    const ResampleAxis ay = resample_axis(d.in_h, d.out_h);
    float* o = out + (long)b * 3 * plane;
#pragma omp parallel for schedule(static) num_threads(nt)
    for (int Y = 0; Y < pad_h; ++Y) {
      const int yy = d.flip_v ? d.out_h - 1 - Y : Y;
      for (int X = 0; X < pad_w; ++X) {
        float* px = o + (long)Y * pad_w + X;
        if (Y >= d.out_h || X >= d.out_w) {
          px[0] = px[plane] = px[2 * plane] = 0.f;
          continue;
        }
        const int xx = d.flip_h ? d.out_w - 1 - X : X;
        const uint8_t* col = src + 3L * xx;
        int u[3];
        if (d.out_h != d.in_h) {
          resample_position([&](int i, int c) { return (int)col[i * stride + c]; }, ay, d.in_h, yy, u);
        } else {
          for (int c = 0; c < 3; ++c) u[c] = col[yy * stride + c];
        }
        for (int c = 0; c < 3; ++c) px[c * plane] = normalized_channel(u, c, to_bgr255, mean, std);
      }
    }
  }
  return OVIS_CPU_OK;
}

// ---- the windowed input transform: host twin of ovis_transform_images_window_u8 (csrc/image_transform.hip).  The horizontal
// pass runs over the columns the window shows and the input rows its rows read, at the positions of the full resize.
extern "C" int ovis_cpu_transform_images_window_u8(const uint8_t* data, long data_bytes, const int32_t* desc, int batch,
                                                   const float* mean, const float* std, int to_bgr255, int pad_h, int pad_w,
                                                   float* out, int threads) {
  if (batch < 0 || pad_h <= 0 || pad_w <= 0 || data_bytes < 0) return OVIS_CPU_EINVAL;
  if (batch == 0) return OVIS_CPU_OK;
  if (!data || !desc || !mean || !std || !out) return OVIS_CPU_EINVAL;
  if (pad_h > kResampleMaxDim || pad_w > kResampleMaxDim || batch > 65535) return OVIS_CPU_ERANGE;
  auto load = [&](int b) {
    const int32_t* d = desc + (long)b * kWindowDescInts;
    return WindowDesc{ImageDesc{d[0], d[1], d[2], d[3], d[4], d[5], d[6]}, d[7], d[8], d[9], d[10]};
  };
  for (int b = 0; b < batch; ++b) {
    const WindowDesc w = load(b);
    if (w.im.in_h > kResampleMaxDim || w.im.in_w > kResampleMaxDim || w.im.out_h > kResampleMaxDim ||
        w.im.out_w > kResampleMaxDim)
      return OVIS_CPU_ERANGE;
    if (!window_desc_valid(w, data_bytes, kResampleMaxDim, kResampleMaxDim, pad_h, pad_w)) return OVIS_CPU_EINVAL;
  }
  const long plane = (long)pad_h * pad_w;
  const int nt = thread_count(threads);
  for (int b = 0; b < batch; ++b) {
    const WindowDesc w = load(b);
    const ImageDesc d = w.im;
    const uint8_t* src = data + d.offset;
    const int x0 = window_first_col(w);
    int lo, hi;
    window_input_rows(w, &lo, &hi);
    // horizontal pass -> uint8 [in_h, win_w, 3], rows [lo, hi) only; skipped when the width does not change
    std::vector<uint8_t> rows;
    long stride = 3L * d.in_w;
    long first = 3L * x0;  // of the window's first column in a row of `src`
    if (d.out_w != d.in_w) {
      rows.resize(3UL * d.in_h * w.win_w);
      stride = 3L * w.win_w;
      first = 0;
      const ResampleAxis ax = resample_axis(d.in_w, d.out_w);
#pragma omp parallel for schedule(static) num_threads(nt)
      for (int j = 0; j < w.win_w; ++j) {
        for (int y = lo; y < hi; ++y) {
          const uint8_t* row = src + 3L * y * d.in_w;
          int u[3];
          resample_position([&](int i, int c) { return (int)row[3 * i + c]; }, ax, d.in_w, x0 + j, u);
          for (int c = 0; c < 3; ++c) rows[y * stride + 3L * j + c] = (uint8_t)u[c];
        }
      }
      src = rows.data();
    }
    const ResampleAxis ay = resample_axis(d.in_h, d.out_h);
    float* o = out + (long)b * 3 * plane;
#pragma omp parallel for schedule(static) num_threads(nt)
    for (int Y = 0; Y < pad_h; ++Y) {
      const int fy = w.win_y + Y;
      const int yy = d.flip_v ? d.out_h - 1 - fy : fy;
      for (int X = 0; X < pad_w; ++X) {
        float* px = o + (long)Y * pad_w + X;
        if (Y >= w.win_h || X >= w.win_w) {
          px[0] = px[plane] = px[2 * plane] = 0.f;
          continue;
        }
        const int fx = w.win_x + X;
        const int xx = d.flip_h ? d.out_w - 1 - fx : fx;
        const uint8_t* col = src + first + 3L * (xx - x0);
        int u[3];
        if (d.out_h != d.in_h) {
          resample_position([&](int i, int c) { return (int)col[i * stride + c]; }, ay, d.in_h, yy, u);
        } else {
          for (int c = 0; c < 3; ++c) u[c] = col[yy * stride + c];
        }
        for (int c = 0; c < 3; ++c) px[c * plane] = normalized_channel(u, c, to_bgr255, mean, std);
      }
    }
  }
  return OVIS_CPU_OK;
}

// ---- colour jitter: host twin of ovis_color_jitter_u8(csrc/color_jitter.hip), the arithmetic of color_jitter_chain.h ------------
extern "C" int ovis_cpu_color_jitter_u8(const uint8_t* data, long data_bytes, const int32_t* desc, const int32_t* ops,
                                        const float* params, int batch, uint8_t* out, int threads) {
  if (batch < 0 || data_bytes < 0) return OVIS_CPU_EINVAL;
  if (batch == 0) return OVIS_CPU_OK;
  if (!data || !desc || !ops || !params || !out) return OVIS_CPU_EINVAL;
  if ((uintptr_t)data < (uintptr_t)out + (uintptr_t)data_bytes && (uintptr_t)out < (uintptr_t)data + (uintptr_t)data_bytes)
    return OVIS_CPU_EINVAL;
  if (batch > 65535) return OVIS_CPU_ERANGE;
  for (int b = 0; b < batch; ++b) {
    const int32_t* d = desc + (long)b * kImageDescInts;
    if (d[1] > kResampleMaxDim || d[2] > kResampleMaxDim) return OVIS_CPU_ERANGE;
    if (!jitter_desc_in_buffer(d[0], d[1], d[2], data_bytes, kResampleMaxDim, kResampleMaxDim)) return OVIS_CPU_EINVAL;
  }
  const int nt = thread_count(threads);
  for (int b = 0; b < batch; ++b) {
    const int32_t* d = desc + (long)b * kImageDescInts;
    const uint8_t* src = data + d[0];
    uint8_t* dst = out + d[0];
    const long pixels = (long)d[1] * d[2];
    const JitterChain c = jitter_chain(ops + (long)b * kJitterSlots, params + (long)b * kJitterSlots);
    if (c.n <= 0) {  // no operation, or a malformed row: a copy
      std::memcpy(dst, src, 3 * (size_t)pixels);
      continue;
    }
    int mean = 0;
    if (c.contrast < c.n) {
      long sum = 0;
#pragma omp parallel for schedule(static) num_threads(nt) reduction(+ : sum)
      for (long p = 0; p < pixels; ++p) {
        int rgb[3] = {src[3 * p], src[3 * p + 1], src[3 * p + 2]};
        jitter_apply(c, c.contrast, 0, rgb);
        sum += jitter_grey(rgb);
      }
      mean = jitter_contrast_mean(sum, pixels);
    }
#pragma omp parallel for schedule(static) num_threads(nt)
    for (long p = 0; p < pixels; ++p) {
      int rgb[3] = {src[3 * p], src[3 * p + 1], src[3 * p + 2]};
      jitter_apply(c, c.n, mean, rgb);
      for (int k = 0; k < 3; ++k) dst[3 * p + k] = (uint8_t)rgb[k];
    }
  }
  return OVIS_CPU_OK;
}

// ---- the prediction compositor: host twin of ovis_render_instances_u8 (csrc/render.hip), the arithmetic of pasted_value.h and
// render_geom.h.  The device kernel walks the pixels and, per pixel, the layers in order; here the layers are walked in
// order and, per layer, the pixels of its clipped box -- the same sequence of updates for every pixel.
extern "C" int ovis_cpu_render_instances_u8(const uint8_t* image, int height, int width, const float* maps, const float* boxes,
                                            int num_layers, int map_resolution, const int32_t* kinds, const float* params,
                                            const float* colors, float alpha, const uint8_t* outline_colors,
                                            int outline_thickness, uint8_t* out, int threads) {
  if (height <= 0 || width <= 0 || num_layers < 0 || !image || !out || !(alpha >= 0.f && alpha <= 1.f)) return OVIS_CPU_EINVAL;
  if (num_layers > 0 && (map_resolution <= 0 || !maps || !boxes || !kinds || !params || !colors)) return OVIS_CPU_EINVAL;
  if (num_layers > 0 && outline_colors && outline_thickness < 1) return OVIS_CPU_EINVAL;
  if (height > kRenderMaxDim || width > kRenderMaxDim) return OVIS_CPU_ERANGE;
  const long bytes = 3L * height * width;
  if ((uintptr_t)image < (uintptr_t)out + bytes && (uintptr_t)out < (uintptr_t)image + bytes) return OVIS_CPU_EINVAL;
  if (num_layers > 0 && map_resolution > 120) return OVIS_CPU_ERANGE;  // the device entry's LDS limit
  if (num_layers > 0 && outline_colors && outline_thickness > kRenderMaxThickness) return OVIS_CPU_ERANGE;
  std::memcpy(out, image, (size_t)bytes);
  const int nt = thread_count(threads);
  const int M = map_resolution, S = M + 2, W = width, H = height;
  if (outline_colors) {
    const int lo = outline_thickness / 2, hi = (outline_thickness + 1) / 2 - 1;
    for (int i = 0; i < num_layers; ++i) {
      const float* gb = boxes + 4L * i;
      if (!render_box_sane(gb[0], gb[1], gb[2], gb[3])) continue;
      const OutlineRect r = outline_rect(gb[0], gb[1], gb[2], gb[3]);
      const long ya = std::max<long>((long)r.ya - lo, 0), yb = std::min<long>((long)r.yb + hi, H - 1);
      const long xa = std::max<long>((long)r.xa - lo, 0), xb = std::min<long>((long)r.xb + hi, W - 1);
      for (long Y = ya; Y <= yb; ++Y)
        for (long X = xa; X <= xb; ++X)
          if (outline_covers(r, lo, hi, (int)Y, (int)X)) std::memcpy(out + (Y * W + X) * 3, outline_colors + 3L * i, 3);
    }
  }
  std::vector<float> padded((size_t)(num_layers > 0 ? S * S : 0));
  const double a = (double)alpha;
  for (int i = 0; i < num_layers; ++i) {
    const int kind = kinds[i];
    if (kind != kRenderFill && kind != kRenderHeat) continue;
    const float* gb = boxes + 4L * i;
    if (!render_box_sane(gb[0], gb[1], gb[2], gb[3])) continue;
    const PastedRect r = pasted_rect(gb[0], gb[1], gb[2], gb[3], M);
    const int cx0 = std::max(r.x0, 0), cx1 = std::min(r.x1, W - 1), cy0 = std::max(r.y0, 0), cy1 = std::min(r.y1, H - 1);
    if (cx1 < cx0 || cy1 < cy0) continue;
    std::fill(padded.begin(), padded.end(), 0.f);
    for (int y = 0; y < M; ++y) std::memcpy(&padded[(size_t)(y + 1) * S + 1], maps + ((long)i * M + y) * M, sizeof(float) * M);
    const float* pd = padded.data();
    auto at = [&](int y, int x) { return pd[y * S + x]; };
    const float param = params[i];
    const float* col = colors + 3L * i;
#pragma omp parallel for schedule(static) num_threads(nt)
    for (int Y = cy0; Y <= cy1; ++Y) {
      for (int X = cx0; X <= cx1; ++X) {
        uint8_t* px = out + ((long)Y * W + X) * 3;
        const float v = pasted_value(at, M, r.x0, r.y0, r.bw, r.bh, Y, X);
        if (kind == kRenderFill) {
          if (v > param)
            for (int c = 0; c < 3; ++c) px[c] = (uint8_t)render_fill(px[c], col[c], a);
        } else {
          const float m = render_heat_weight(v, param);
          if (m != 0.f)
            for (int c = 0; c < 3; ++c) px[c] = (uint8_t)render_heat(px[c], m, col[c]);
        }
      }
    }
  }
  return OVIS_CPU_OK;
}

// ---- box voting over the merged candidate list and the mean of the views' mask maps (not in the reference) --------------------
// Twin of csrc/box_vote.hip: the IoU is ovis_cpu_nms_f32's (= nms.hip's) expression; lane l of 64 sums the voters lo + l,
// lo + l + 64, ... in that order and the lanes are folded by the xor butterfly 32, 16, ... 1, as the wavefront does.
extern "C" int ovis_cpu_vote_boxes_f32(const float* cand_boxes, const float* cand_scores, const int32_t* offsets,
                                       const int32_t* cand_group, long num_candidates, int num_groups, const int64_t* kept,
                                       long num_kept, float vote_thresh, float* voted) {
  if (num_candidates < 0 || num_groups < 0 || num_kept < 0) return OVIS_CPU_EINVAL;
  if (num_kept == 0) return OVIS_CPU_OK;
  if (!kept || !voted || !offsets) return OVIS_CPU_EINVAL;
  if (num_candidates > 0 && (!cand_boxes || !cand_scores || !cand_group)) return OVIS_CPU_EINVAL;
  int bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(| : bad)
  for (long j = 0; j < num_kept; ++j) {
    float* out = voted + 4 * j;
    out[0] = out[1] = out[2] = out[3] = 0.f;
    const int64_t d = kept[j];
    if (d < 0 || d >= num_candidates) { bad |= 1; continue; }
    const int g = cand_group[d];
    if (g < 0 || g >= num_groups) { bad |= 1; continue; }
    const long lo = offsets[g], hi = offsets[g + 1];
    if (lo < 0 || hi > num_candidates || d < lo || d >= hi) { bad |= 1; continue; }
    const float* a = cand_boxes + 4 * d;
    const float area_a = (a[2] - a[0] + 1.f) * (a[3] - a[1] + 1.f);
    float part[5][64];
    for (int c = 0; c < 5; ++c)
      for (int l = 0; l < 64; ++l) part[c][l] = 0.f;
    for (long k = lo; k < hi; ++k) {
      const float* b = cand_boxes + 4 * k;
      const float left = std::max(a[0], b[0]), right = std::min(a[2], b[2]);
      const float top = std::max(a[1], b[1]), bottom = std::min(a[3], b[3]);
      const float w = std::max(right - left + 1.f, 0.f), h = std::max(bottom - top + 1.f, 0.f);
      const float inter = w * h;
      const float area_b = (b[2] - b[0] + 1.f) * (b[3] - b[1] + 1.f);
      if (!(inter / (area_a + area_b - inter) >= vote_thresh)) continue;
      const int l = (int)((k - lo) & 63);
      const float s = cand_scores[k];
      part[0][l] = part[0][l] + s;
      for (int c = 0; c < 4; ++c) part[c + 1][l] = part[c + 1][l] + s * b[c];
    }
    for (int c = 0; c < 5; ++c)
      for (int off = 32; off > 0; off >>= 1) {
        float next[64];
        for (int l = 0; l < 64; ++l) next[l] = part[c][l] + part[c][l ^ off];
        for (int l = 0; l < 64; ++l) part[c][l] = next[l];
      }
    for (int c = 0; c < 4; ++c) out[c] = part[c + 1][0] / part[0][0];
  }
  return bad ? OVIS_CPU_ERANGE : OVIS_CPU_OK;
}

extern "C" int ovis_cpu_average_view_masks_f32(const float* maps, int num_views, long num_maps, int resolution,
                                               uint64_t flip_bits, float* out) {
  if (num_views < 1 || num_maps < 0 || resolution < 1) return OVIS_CPU_EINVAL;
  if (num_views > 64 || resolution > 32768) return OVIS_CPU_ERANGE;
  const long M = resolution, rows = num_maps * M, per_view = rows * M;
  if (per_view == 0) return OVIS_CPU_OK;
  if (!maps || !out) return OVIS_CPU_EINVAL;
  const float count = (float)num_views;
#pragma omp parallel for schedule(static)
  for (long r = 0; r < rows; ++r)
    for (long x = 0; x < M; ++x) {
      const long i = r * M + x, mirrored = r * M + (M - 1 - x);
      float acc = maps[(flip_bits & 1ull) ? mirrored : i];
      for (int v = 1; v < num_views; ++v) acc = acc + maps[v * per_view + (((flip_bits >> v) & 1ull) ? mirrored : i)];
      out[i] = acc / count;
    }
  return OVIS_CPU_OK;
}

// ---- Soft-NMS over the (image, class) runs of a candidate list (not in the reference; the rule: include/ovis_hip.h) ------------
// Twin of csrc/soft_nms.hip as a plain loop: per round the alive candidate with the largest working score (ascending scan
// and a strict >: the lower index wins a tie), then the decay of the others.  The same float32 operations on the same operands
// (the IoU is nms.hip's expression, the Gaussian weight a float64 exponential rounded once), so the bits agree.
constexpr int kSoftNmsLinear = 0, kSoftNmsGaussian = 1, kSoftNmsHard = 2;   // the values of OVIS_SOFT_NMS_* (include/ovis_hip.h)

extern "C" int ovis_cpu_soft_nms_f32(const float* cand_boxes, const float* cand_scores, const int32_t* offsets,
                                     long num_candidates, int num_groups, int method, float nms_thresh, float sigma,
                                     float min_score, float* soft_scores) {
  if (num_candidates < 0 || num_groups < 0) return OVIS_CPU_EINVAL;
  if (method != kSoftNmsLinear && method != kSoftNmsGaussian && method != kSoftNmsHard)
    return OVIS_CPU_EINVAL;
  if (!(sigma > 0.f) || !(min_score >= 0.f)) return OVIS_CPU_EINVAL;
  if (num_candidates == 0 || num_groups == 0) return OVIS_CPU_OK;
  if (!cand_boxes || !cand_scores || !offsets || !soft_scores) return OVIS_CPU_EINVAL;
  // the runs in front of the first pair that is not well-formed; every candidate behind them gets 0
  int good = 0;
  while (good < num_groups && (good == 0 ? offsets[0] == 0 : offsets[good] >= 0) && offsets[good] <= offsets[good + 1] &&
         (long)offsets[good + 1] <= num_candidates)
    ++good;
  const long covered = good == 0 ? 0 : (long)offsets[good];
  for (long k = covered; k < num_candidates; ++k) soft_scores[k] = 0.f;
#pragma omp parallel for schedule(dynamic, 4)
  for (int g = 0; g < good; ++g) {
    const long lo = offsets[g];
    const int n = offsets[g + 1] - offsets[g];
    const float* boxes = cand_boxes + 4 * lo;
    float* out = soft_scores + lo;
    std::vector<float> w(cand_scores + lo, cand_scores + lo + n);
    for (int k = 0; k < n; ++k)
      if (!(w[k] > 0.f)) w[k] = out[k] = 0.f;   // w > 0 iff alive
    for (;;) {
      int m = -1;
      float top = 0.f;
      for (int k = 0; k < n; ++k)
        if (w[k] > top) { top = w[k]; m = k; }
      if (m < 0) break;
      out[m] = top;
      w[m] = 0.f;
      const float* a = boxes + 4 * m;
      const float area_a = (a[2] - a[0] + 1.f) * (a[3] - a[1] + 1.f);
      for (int k = 0; k < n; ++k) {
        if (!(w[k] > 0.f)) continue;
        const float* b = boxes + 4 * k;
        const float left = std::max(a[0], b[0]), right = std::min(a[2], b[2]);
        const float up = std::max(a[1], b[1]), bottom = std::min(a[3], b[3]);
        const float width = std::max(right - left + 1.f, 0.f), height = std::max(bottom - up + 1.f, 0.f);
        const float inter = width * height;
        const float area_b = (b[2] - b[0] + 1.f) * (b[3] - b[1] + 1.f);
        const float ov = inter / (area_a + area_b - inter);
        float weight = 1.f;
        if (method == kSoftNmsGaussian) {
          const float q = (ov * ov) / sigma;
          weight = (float)std::exp(-(double)q);
        } else if (ov > nms_thresh) {
          weight = method == kSoftNmsLinear ? 1.f - ov : 0.f;
        }
        const float v = w[k] * weight;
        if (v >= min_score && v > 0.f) w[k] = v;
        else w[k] = out[k] = 0.f;
      }
    }
  }
  return (good < num_groups || covered != num_candidates) ? OVIS_CPU_ERANGE : OVIS_CPU_OK;
}

extern "C" const char* ovis_cpu_version(void) { return "ovis_cpu 7 (RoIAlign fwd/bwd, NMS, polygon masks and mask targets, input transform, prediction compositor, box voting and view-averaged masks, Soft-NMS; fp32, OpenMP)"; }
