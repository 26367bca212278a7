// The input transform on the device: B raw RGB uint8 images of different sizes -> the padded fp32 batch [B, 3, pad_h, pad_w]
// the step reads (mb/data/transforms/transforms.py:27-62 Resize, :65-85 flips, :105-120 ToTensor + Normalize;
// mb/structures/image_list.py:29-70 zero padding), bit for bit what the reference computes per image on the host with PIL.
//
// PIL's bilinear resize is two 8-bit passes, horizontal then vertical, and the 8-bit rounding BETWEEN them is part of the
// result.  Two launches per batch, whatever B:
//   1. transform_rows_kernel: every image whose width changes -> uint8 [in_h, out_w, 3] in the workspace (a thread owns one
//      intermediate pixel, three channels; 3 bytes per lane, consecutive lanes consecutive pixels);
//   2. transform_finish_kernel: EVERY element of out exactly once -- the vertical pass over the intermediate (or over the
//      input itself when the width did not change), the flips as a reversed read position, channel order, (v - mean) / std,
//      zeros outside out_h x out_w.  A thread owns one (y, x) and stores its three planes; consecutive lanes consecutive x.
// A fused tile through LDS would need the intermediate rows [ymin(first row), ymax(last row)) of a tile resident, and a
// downscaling axis has no bound on that short of in_h; the workspace has one code path for every size, is 1.5 MB per
// 480 x 640 -> 800 x 1066 image next to the 10 MB of output the batch is bound by, and is re-read from cache.
// The tap weights are recomputed per thread in fp64 (resample_geom.h): no per-image table crosses PCIe.
//
// The descriptors live on the device and are never read back; the host checks the bounds it is given (max_in_h, max_in_w,
// pad_h, pad_w), and an image whose descriptor does not fit them or the byte buffer comes out as NaN, untouched otherwise.
//
// A second pair of kernels (ovis_transform_images_window_u8, below) makes a crop window of the resized, flipped image for
// scale jitter with a fixed-size crop, without materialising the resized image.
#include "ovis_common.h"

#define OVIS_HD __host__ __device__ __forceinline__
#include "resample_geom.h"

namespace {

constexpr int kTransformThreads = 256;

struct TransformParams {
  float mean[3], std[3];
  int to_bgr255;
};

__device__ __forceinline__ ImageDesc load_desc(const int* __restrict__ desc, int b) {
  const int* d = desc + (long)b * kImageDescInts;
  return ImageDesc{d[0], d[1], d[2], d[3], d[4], d[5], d[6]};
}

__global__ __launch_bounds__(kTransformThreads) void transform_rows_kernel(const unsigned char* __restrict__ data,
                                                                           long data_bytes, const int* __restrict__ desc,
                                                                           int max_in_h, int max_in_w, int pad_h, int pad_w,
                                                                           unsigned char* __restrict__ ws) {
  const int b = blockIdx.z, y = blockIdx.y, x = blockIdx.x * kTransformThreads + threadIdx.x;
  const ImageDesc d = load_desc(desc, b);
  if (!image_desc_valid(d, data_bytes, max_in_h, max_in_w, pad_h, pad_w)) return;
  if (d.out_w == d.in_w || y >= d.in_h || x >= d.out_w) return;  // y < in_h <= max_in_h, x < out_w <= pad_w
  const unsigned char* row = data + d.offset + 3L * y * d.in_w;
  int u[3];
  resample_position([&](int i, int c) { return (int)row[3 * i + c]; }, resample_axis(d.in_w, d.out_w), d.in_w, x, u);
  unsigned char* o = ws + 3L * (((long)b * max_in_h + y) * pad_w + x);
  o[0] = (unsigned char)u[0];
  o[1] = (unsigned char)u[1];
  o[2] = (unsigned char)u[2];
}

__global__ __launch_bounds__(kTransformThreads) void transform_finish_kernel(const unsigned char* __restrict__ data,
                                                                             long data_bytes, const int* __restrict__ desc,
                                                                             int max_in_h, int max_in_w, int pad_h, int pad_w,
                                                                             const unsigned char* __restrict__ ws,
                                                                             TransformParams p, float* __restrict__ out) {
  const int b = blockIdx.z, Y = blockIdx.y, X = blockIdx.x * kTransformThreads + threadIdx.x;
  if (X >= pad_w) return;  // Y < pad_h: the grid's y extent
  const ImageDesc d = load_desc(desc, b);
  const long plane = (long)pad_h * pad_w;
  float* o = out + (long)b * 3 * plane + (long)Y * pad_w + X;
  if (!image_desc_valid(d, data_bytes, max_in_h, max_in_w, pad_h, pad_w)) {
    o[0] = o[plane] = o[2 * plane] = __builtin_nanf("");
    return;
  }
  if (Y >= d.out_h || X >= d.out_w) {
    o[0] = o[plane] = o[2 * plane] = 0.f;
    return;
  }
  // F.hflip / F.vflip of the resized image: position (Y, X) shows its pixel (out_h - 1 - Y, out_w - 1 - X)
  const int yy = d.flip_v ? d.out_h - 1 - Y : Y, xx = d.flip_h ? d.out_w - 1 - X : X;
  // the rows the vertical pass reads: the intermediate, or the image itself when the horizontal pass was skipped
  const bool resized_w = d.out_w != d.in_w;
  const unsigned char* col = resized_w ? ws + 3L * ((long)b * max_in_h * pad_w + xx) : data + d.offset + 3L * xx;
  const long stride = 3L * (resized_w ? pad_w : d.in_w);
  int u[3];
  if (d.out_h != d.in_h) {
    resample_position([&](int i, int c) { return (int)col[i * stride + c]; }, resample_axis(d.in_h, d.out_h), d.in_h, yy, u);
  } else {
    for (int c = 0; c < 3; ++c) u[c] = col[yy * stride + c];
  }
  for (int c = 0; c < 3; ++c) o[c * plane] = normalized_channel(u, c, p.to_bgr255, p.mean, p.std);
}

// ---- the windowed form: scale jitter + fixed-size crop (ovis_transform_images_window_u8) ---------------------------------
// The same two launches over 11-int descriptors.  The canvas shows the window [win_y, win_y + win_h) x [win_x, win_x + win_w)
// of the resized, flipped image; out_h x out_w (up to 16384, whatever the canvas) is never materialised:
//   1. transform_window_rows_kernel: intermediate pixel (y, j), j < win_w, is column window_first_col + j of the horizontal
//      pass over input row y -- only the columns the window shows, and only the input rows [lo, hi) of window_input_rows,
//      the ones its rows read in the vertical pass.  Row y of image b lives where the un-windowed form keeps it, so the
//      workspace is batch * max_in_h * pad_w * 3 bytes whatever the scale;
//   2. transform_window_finish_kernel: every element of out once -- (Y, X) inside win_h x win_w is pixel (win_y + Y,
//      win_x + X) of the flipped image, zero elsewhere.
// The arithmetic is resample_geom.h's with the positions of the full out_h x out_w resize, so a pixel has the bits of the
// same window sliced out of transform_finish_kernel's output.
__device__ __forceinline__ WindowDesc load_window_desc(const int* __restrict__ desc, int b) {
  const int* d = desc + (long)b * kWindowDescInts;
  return WindowDesc{ImageDesc{d[0], d[1], d[2], d[3], d[4], d[5], d[6]}, d[7], d[8], d[9], d[10]};
}

__global__ __launch_bounds__(kTransformThreads) void transform_window_rows_kernel(
    const unsigned char* __restrict__ data, long data_bytes, const int* __restrict__ desc, int max_in_h, int max_in_w,
    int pad_h, int pad_w, unsigned char* __restrict__ ws) {
  const int b = blockIdx.z, y = blockIdx.y, j = blockIdx.x * kTransformThreads + threadIdx.x;
  const WindowDesc w = load_window_desc(desc, b);
  if (!window_desc_valid(w, data_bytes, max_in_h, max_in_w, pad_h, pad_w)) return;
  const ImageDesc d = w.im;
  if (d.out_w == d.in_w || j >= w.win_w) return;  // j < win_w <= pad_w
  int lo, hi;
  window_input_rows(w, &lo, &hi);
  if (y < lo || y >= hi) return;  // 0 <= lo, hi <= in_h <= max_in_h
  const unsigned char* row = data + d.offset + 3L * y * d.in_w;
  int u[3];
  resample_position([&](int i, int c) { return (int)row[3 * i + c]; }, resample_axis(d.in_w, d.out_w), d.in_w,
                    window_first_col(w) + j, u);  // a column of the full resize: first_col + j < out_w
  unsigned char* o = ws + 3L * (((long)b * max_in_h + y) * pad_w + j);
  o[0] = (unsigned char)u[0];
  o[1] = (unsigned char)u[1];
  o[2] = (unsigned char)u[2];
}

__global__ __launch_bounds__(kTransformThreads) void transform_window_finish_kernel(
    const unsigned char* __restrict__ data, long data_bytes, const int* __restrict__ desc, int max_in_h, int max_in_w,
    int pad_h, int pad_w, const unsigned char* __restrict__ ws, TransformParams p, float* __restrict__ out) {
  const int b = blockIdx.z, Y = blockIdx.y, X = blockIdx.x * kTransformThreads + threadIdx.x;
  if (X >= pad_w) return;  // Y < pad_h: the grid's y extent
  const WindowDesc w = load_window_desc(desc, b);
  const long plane = (long)pad_h * pad_w;
  float* o = out + (long)b * 3 * plane + (long)Y * pad_w + X;
  if (!window_desc_valid(w, data_bytes, max_in_h, max_in_w, pad_h, pad_w)) {
    o[0] = o[plane] = o[2 * plane] = __builtin_nanf("");
    return;
  }
  if (Y >= w.win_h || X >= w.win_w) {
    o[0] = o[plane] = o[2 * plane] = 0.f;
    return;
  }
  const ImageDesc d = w.im;
  // position (win_y + Y, win_x + X) of the flipped image shows pixel (yy, xx) of the resized one; xx - window_first_col is
  // its column in the intermediate
  const int fy = w.win_y + Y, fx = w.win_x + X;
  const int yy = d.flip_v ? d.out_h - 1 - fy : fy, xx = d.flip_h ? d.out_w - 1 - fx : fx;
  const bool resized_w = d.out_w != d.in_w;
  const unsigned char* col =
      resized_w ? ws + 3L * ((long)b * max_in_h * pad_w + (xx - window_first_col(w))) : data + d.offset + 3L * xx;
  const long stride = 3L * (resized_w ? pad_w : d.in_w);
  int u[3];
  if (d.out_h != d.in_h) {  // reads rows inside window_input_rows: the ones the first launch wrote
    resample_position([&](int i, int c) { return (int)col[i * stride + c]; }, resample_axis(d.in_h, d.out_h), d.in_h, yy, u);
  } else {
    for (int c = 0; c < 3; ++c) u[c] = col[yy * stride + c];
  }
  for (int c = 0; c < 3; ++c) o[c * plane] = normalized_channel(u, c, p.to_bgr255, p.mean, p.std);
}

}  // namespace

extern "C" size_t ovis_transform_images_window_workspace_bytes(int batch, int max_in_h, int pad_w) {
  if (batch <= 0 || max_in_h <= 0 || pad_w <= 0) return 0;
  return (size_t)batch * (size_t)max_in_h * (size_t)pad_w * 3;
}

extern "C" int ovis_transform_images_window_u8(const uint8_t* data, long data_bytes, const int32_t* desc, int batch,
                                               int max_in_h, int max_in_w, const float* mean, const float* std,
                                               int to_bgr255, int pad_h, int pad_w, void* workspace, size_t workspace_bytes,
                                               float* out, void* stream) {
  if (batch < 0 || max_in_h <= 0 || max_in_w <= 0 || pad_h <= 0 || pad_w <= 0 || data_bytes < 0) return OVIS_EINVAL;
  if (batch == 0) return OVIS_OK;
  if (!data || !desc || !mean || !std || !out) return OVIS_EINVAL;
  if (max_in_h > kResampleMaxDim || max_in_w > kResampleMaxDim || pad_h > kResampleMaxDim || pad_w > kResampleMaxDim ||
      batch > 65535)
    return OVIS_ERANGE;
  if (!workspace || workspace_bytes < ovis_transform_images_window_workspace_bytes(batch, max_in_h, pad_w)) return OVIS_ENOSPC;
  TransformParams p;
  for (int c = 0; c < 3; ++c) {
    p.mean[c] = mean[c];
    p.std[c] = std[c];
  }
  p.to_bgr255 = to_bgr255;
  const unsigned bx = (unsigned)ovis_ceil_div(pad_w, kTransformThreads);
  hipLaunchKernelGGL(transform_window_rows_kernel, dim3(bx, (unsigned)max_in_h, (unsigned)batch), dim3(kTransformThreads), 0,
                     (hipStream_t)stream, (const unsigned char*)data, data_bytes, (const int*)desc, max_in_h, max_in_w, pad_h,
                     pad_w, (unsigned char*)workspace);
  OVIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(transform_window_finish_kernel, dim3(bx, (unsigned)pad_h, (unsigned)batch), dim3(kTransformThreads), 0,
                     (hipStream_t)stream, (const unsigned char*)data, data_bytes, (const int*)desc, max_in_h, max_in_w, pad_h,
                     pad_w, (const unsigned char*)workspace, p, out);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}

extern "C" size_t ovis_transform_images_workspace_bytes(int batch, int max_in_h, int pad_w) {
  if (batch <= 0 || max_in_h <= 0 || pad_w <= 0) return 0;
  return (size_t)batch * (size_t)max_in_h * (size_t)pad_w * 3;
}

extern "C" int ovis_transform_images_u8(const uint8_t* data, long data_bytes, const int32_t* desc, int batch, int max_in_h,
                                        int max_in_w, const float* mean, const float* std, int to_bgr255, int pad_h,
                                        int pad_w, void* workspace, size_t workspace_bytes, float* out, void* stream) {
  if (batch < 0 || max_in_h <= 0 || max_in_w <= 0 || pad_h <= 0 || pad_w <= 0 || data_bytes < 0) return OVIS_EINVAL;
  if (batch == 0) return OVIS_OK;
  if (!data || !desc || !mean || !std || !out) return OVIS_EINVAL;
  if (max_in_h > kResampleMaxDim || max_in_w > kResampleMaxDim || pad_h > kResampleMaxDim || pad_w > kResampleMaxDim ||
      batch > 65535)
    return OVIS_ERANGE;
  if (!workspace || workspace_bytes < ovis_transform_images_workspace_bytes(batch, max_in_h, pad_w)) return OVIS_ENOSPC;
  TransformParams p;
  for (int c = 0; c < 3; ++c) {
    p.mean[c] = mean[c];
    p.std[c] = std[c];
  }
  p.to_bgr255 = to_bgr255;
  const unsigned bx = (unsigned)ovis_ceil_div(pad_w, kTransformThreads);
  hipLaunchKernelGGL(transform_rows_kernel, dim3(bx, (unsigned)max_in_h, (unsigned)batch), dim3(kTransformThreads), 0,
                     (hipStream_t)stream, (const unsigned char*)data, data_bytes, (const int*)desc, max_in_h, max_in_w, pad_h,
                     pad_w, (unsigned char*)workspace);
  OVIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(transform_finish_kernel, dim3(bx, (unsigned)pad_h, (unsigned)batch), dim3(kTransformThreads), 0,
                     (hipStream_t)stream, (const unsigned char*)data, data_bytes, (const int*)desc, max_in_h, max_in_w, pad_h,
                     pad_w, (const unsigned char*)workspace, p, out);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}
