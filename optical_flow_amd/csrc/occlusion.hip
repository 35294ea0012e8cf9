// Occlusion masks of the image warp convention, every pyramid level in one launch: for each
// pixel of image 1 whether the data terms may score it (1.0f) or not (0.0f).
//   x = j + f0, y = i + f1   (the sample point warp_tap<WARP_CV_IMAGE> forms, in fp32)
//   border: 0 <= x <= w-1 and 0 <= y <= h-1 (inclusive)
//   fb:     border, and with g~ the partner image's flow sampled bilinearly at (x, y)
//           |f + g~|^2 <= alpha1 * (|f|^2 + |g~|^2) + alpha2[l]
// Image b's partner is (b + pair_stride) % n: images [0,B) hold the forward flows, [B,2B) the
// flows of the same pairs swapped.  Pixelwise: a grid-stride loop over all levels' pixels, one
// float stored per pixel, no atomics, nothing differentiates through the result.
#include <algorithm>

#include "loss_levels.h"
#include "warp_tap.h"

namespace oflow {

// Level l's pixels are [beg[l], beg[l+1]).
struct OccMulti : LevelTable {
  const float* flow[8];
  float* mask[8];
  float alpha2[8];
};

template <int MODE>
__global__ __launch_bounds__(256) void occ_mask_multi(int n, int pair_stride, float alpha1,
                                                      OccMulti m) {
  const int64_t total = m.beg[m.levels];
  for (int64_t gp = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; gp < total;
       gp += (int64_t)gridDim.x * blockDim.x) {
    const int l = level_of(m, gp);
    const int h = m.h[l], w = m.w[l];
    const float* flow = m.flow[l];
    const int64_t p = gp - m.beg[l];
    const int j = (int)(p % w);
    const int64_t t2 = p / w;
    const int i = (int)(t2 % h);
    const int b = (int)(t2 / h);
    const float2 f = *reinterpret_cast<const float2*>(flow + 2 * p);
    // warp_tap<WARP_CV_IMAGE>'s own x and y
    const float x = (float)j + f.x, y = (float)i + f.y;
    bool ok = x >= 0.f && x <= (float)(w - 1) && y >= 0.f && y <= (float)(h - 1);
    if (MODE == OF_OCC_FB && ok) {
      const int64_t pimg = (int64_t)((b + pair_stride) % n) * h * w;
      const WarpTap t = warp_tap<WARP_CV_IMAGE>(i, j, f.x, f.y, h, w, pimg);
      const float a = t.a, c = t.b;
      const float w00 = a * c, w01 = a * (1.f - c), w10 = (1.f - a) * c,
                  w11 = (1.f - a) * (1.f - c);
      const float2 v0 = *reinterpret_cast<const float2*>(flow + 2 * t.o00);
      const float2 v1 = *reinterpret_cast<const float2*>(flow + 2 * t.o01);
      const float2 v2 = *reinterpret_cast<const float2*>(flow + 2 * t.o10);
      const float2 v3 = *reinterpret_cast<const float2*>(flow + 2 * t.o11);
      const float gx = w00 * v0.x + w01 * v1.x + w10 * v2.x + w11 * v3.x;
      const float gy = w00 * v0.y + w01 * v1.y + w10 * v2.y + w11 * v3.y;
      const float sx = f.x + gx, sy = f.y + gy;
      const float lhs = sx * sx + sy * sy;
      const float rhs = alpha1 * (f.x * f.x + f.y * f.y + gx * gx + gy * gy) + m.alpha2[l];
      ok = lhs <= rhs;
    }
    m.mask[l][p] = ok ? 1.f : 0.f;
  }
}

}  // namespace oflow

using namespace oflow;

extern "C" {

int of_occ_mask_multi(const float* const* flows, int n, int pair_stride, const int* hs,
                      const int* ws, int levels, int mode, float alpha1, const float* alpha2s,
                      float* const* masks, void* stream) {
  static const std::string fn = "of_occ_mask_multi";
  OccMulti m{};
  int st = levels_init(fn, n, hs, ws, levels, m);
  if (st) return st;
  if (!flows || !masks) return fail(OF_EINVAL, fn + ": NULL argument");
  if (mode != OF_OCC_BORDER && mode != OF_OCC_FB) return fail(OF_EINVAL, fn + ": unknown mode");
  if (mode == OF_OCC_FB) {
    if (pair_stride < 1 || (int64_t)n != 2 * (int64_t)pair_stride)
      return fail(OF_EINVAL, fn + ": fb needs n == 2 * pair_stride, pair_stride >= 1");
    if (!(alpha1 >= 0.f)) return fail(OF_EINVAL, fn + ": alpha1 < 0");
    if (!alpha2s) return fail(OF_EINVAL, fn + ": NULL alpha2s");
  } else if (alpha1 < 0.f) {
    return fail(OF_EINVAL, fn + ": alpha1 < 0");
  }
  if ((st = levels_ptrs8(fn, flows, levels, "flow"))) return st;
  for (int l = 0; l < levels; ++l) {
    if (!masks[l]) return fail(OF_EINVAL, fn + ": NULL mask");
    if (mode == OF_OCC_FB && !(alpha2s[l] >= 0.f)) return fail(OF_EINVAL, fn + ": alpha2 < 0");
    m.flow[l] = flows[l];
    m.mask[l] = masks[l];
    m.alpha2[l] = mode == OF_OCC_FB ? alpha2s[l] : 0.f;
  }
  levels_by_pixels(fn, n, m);
  const int grid = grid_for(m.beg[levels]);
  hipLaunchKernelGGL(mode == OF_OCC_FB ? occ_mask_multi<OF_OCC_FB> : occ_mask_multi<OF_OCC_BORDER>,
                     dim3(grid), dim3(256), 0, as_stream(stream), n, pair_stride, alpha1, m);
  return check_launch("occ_mask_multi");
}

}  // extern "C"
