// Image-resolution instance masks from (M x M probability map, box) pairs: the Masker paste (mask_head/inference.py:
// 100-205 with padding 1) of ALL masks of an image in ONE launch.  The reference loops over the masks (pad, expand the
// box, truncate, bilinear resize to the integer box, > threshold, sliced assignment into a zero canvas); here every byte
// of out [P, H, W] is written exactly once, zeros included -- there is no fill followed by a partial paste.
//
// Bound by the HBM write (100 masks at 800 x 1333 = 107 MB; the maps are 78 KB).  A workgroup belongs to ONE mask
// (blockIdx.y) and stages its zero-padded (M+2)^2 map in LDS once; a lane owns 16 consecutive output bytes and stores
// them as one 16-byte word, consecutive lanes consecutive words.  H * W is in general no multiple of 16, so the 16-byte
// words are aligned to the BUFFER, not to the mask or the row: a word may straddle two rows (the lane steps (y, x) per
// byte), and the bytes of a mask in front of its first / behind its last whole word -- the words it shares with its
// neighbours, or the head / tail of the buffer -- are written by that mask's first workgroup with byte stores.  A run
// of 16 bytes that does not meet the integer box is zeros without any arithmetic; inside the box a pixel is
// pasted_inside() of pasted_geom.h, the expressions of project_pasted_masks_kernel (csrc/targets.hip).
#include "ovis_common.h"
#define OVIS_HD __device__ __forceinline__
#include "pasted_geom.h"

namespace {

constexpr int kPasteThreads = 256;
constexpr int kPasteMaxM = 120;  // (M + 2)^2 floats of LDS <= 64 KB

__global__ __launch_bounds__(kPasteThreads) void paste_masks_kernel(const float* __restrict__ probs,
                                                                    const float* __restrict__ boxes, int M, int H, int W,
                                                                    float thr, unsigned char* __restrict__ out) {
  extern __shared__ float padded[];  // [(M+2), (M+2)]: the map inside a zero border of one pixel
  const int p = blockIdx.y, tid = threadIdx.x;
  const int S = M + 2;
  const float* pr = probs + (long)p * M * M;
  for (int i = tid; i < S * S; i += kPasteThreads) {
    const int y = i / S, x = i - y * S;
    padded[i] = (y >= 1 && y <= M && x >= 1 && x <= M) ? pr[(y - 1) * M + (x - 1)] : 0.f;
  }
  __syncthreads();
  const PastedBox pb = pasted_box(*(const float4*)(boxes + 4 * (long)p), M);
  const int4 bx = pb.bx;
  const int bw = pb.bw, bh = pb.bh;
  // the box clipped to the image (inclusive; empty when c?1 < c?0)
  const int cx0 = max(bx.x, 0), cx1 = min(bx.z, W - 1), cy0 = max(bx.y, 0), cy1 = min(bx.w, H - 1);
  auto at = [&](int y, int x) { return padded[y * S + x]; };
  auto pixel = [&](int y, int x) -> unsigned {
    return (y >= cy0 && y <= cy1 && x >= cx0 && x <= cx1 && pasted_inside(at, M, bx, bw, bh, thr, y, x)) ? 1u : 0u;
  };
  const int hw = H * W;
  unsigned char* o = out + (long)p * hw;
  const int head = min((int)((16 - ((uintptr_t)o & 15)) & 15), hw);  // bytes in front of the mask's first aligned word
  const int ngroups = (hw - head) >> 4;
  for (int g = blockIdx.x * kPasteThreads + tid; g < ngroups; g += gridDim.x * kPasteThreads) {
    const int off = head + (g << 4);
    int y = off / W, x = off - y * W;
    const int ye = x + 15 < W ? y : (off + 15) / W;  // row of the run's last byte
    bool meets = cx1 >= cx0 && ye >= cy0 && y <= cy1;
    if (y == ye) meets = meets && x + 15 >= cx0 && x <= cx1;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (meets) {
      unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        w[u >> 2] |= pixel(y, x) << (8 * (u & 3));
        if (++x == W) {
          x = 0;
          ++y;
        }
      }
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *(uint4*)(o + off) = v;
  }
  if (blockIdx.x == 0) {  // the narrow path: < 16 bytes at either end of the mask
    const int tail0 = head + (ngroups << 4);
    if (tid < head) o[tid] = (unsigned char)pixel(tid / W, tid % W);
    const int t = tail0 + tid - 64;
    if (tid >= 64 && t < hw) o[t] = (unsigned char)pixel(t / W, t % W);
  }
}

}  // namespace

extern "C" int ovis_paste_masks_u8(const float* mask_probs, const float* boxes, int num, int prob_resolution,
                                   int image_height, int image_width, float threshold, uint8_t* out, void* stream) {
  if (num < 0 || prob_resolution <= 0 || image_height <= 0 || image_width <= 0) return OVIS_EINVAL;
  if (num == 0) return OVIS_OK;
  if (!mask_probs || !boxes || !out) return OVIS_EINVAL;
  if ((uintptr_t)boxes & 15) return OVIS_ERANGE;
  if (prob_resolution > kPasteMaxM || num > 65535 || (long)image_height * image_width > 0x7fffffefL) return OVIS_ERANGE;
  const int S = prob_resolution + 2;
  const long groups = ((long)image_height * image_width) >> 4;
  // four 16-byte words per lane: ~16 KB of output per workgroup next to the 1 KB map it stages
  const long blocks = (groups + 4 * kPasteThreads - 1) / (4 * kPasteThreads);
  const unsigned bx = (unsigned)(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks));
  hipLaunchKernelGGL(paste_masks_kernel, dim3(bx, (unsigned)num), dim3(kPasteThreads), sizeof(float) * S * S,
                     (hipStream_t)stream, mask_probs, boxes, prob_resolution, image_height, image_width, threshold,
                     (unsigned char*)out);
  OVIS_LAUNCH_CHECK();
  return OVIS_OK;
}
