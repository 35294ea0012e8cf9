// Range-map occlusion masks of the image warp convention (Wang et al., CVPR 2018), every
// pyramid level in one launch per kernel.  The batch is [forward flows ; flows of the same
// pairs swapped]; image b's partner is (b + pair_stride) % n.  Every pixel q = (i, j) of the
// partner's flow g is moved to
//   x = j + g0, y = i + g1   (the sample point warp_tap<WARP_CV_IMAGE> forms, in fp32)
// and splatted bilinearly onto the four pixels around it in image b; a tap outside the frame is
// dropped, a non-finite point contributes nothing.  R_b[p] is the sum of the tap weights that
// land on p, and mask_b[p] = border(f_b)[p] * min(1, R_b[p]) (border: occlusion.hip's own test
// on the pixel's own flow).
//
// The splat is a scatter.  Its sums are integers: each tap weight is quantised to 2^-24 and
// added with a no-return 64-bit atomicAdd into one unsigned long long per destination pixel, so
// the result does not depend on the order in which the adds arrive (warp_det.hip's fixed-point
// path does the same).  64 bits: at this scale a 32-bit sum overflows once 256 sources collapse
// onto a pixel.  Three kernels: zero, splat (one thread per source pixel), finish (one thread
// per destination pixel).  Nothing differentiates through the result.
#include <algorithm>

#include "loss_levels.h"

namespace oflow {

constexpr int RANGE_SHIFT = 24;                       // accumulator unit 2^-24

// Level l's pixels are [beg[l], beg[l+1]); the accumulators are indexed the same way.
struct RangeMulti : LevelTable {
  const float* flow[8];
  float* range[8];
  float* mask[8];
};

__global__ __launch_bounds__(256) void occ_range_zero(unsigned long long* __restrict__ acc,
                                                      int64_t total) {
  for (int64_t gp = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; gp < total;
       gp += (int64_t)gridDim.x * blockDim.x)
    acc[gp] = 0ull;
}

__device__ __forceinline__ void range_tap(unsigned long long* row, bool ok, float wt) {
  if (!ok) return;
  const unsigned long long q = (unsigned long long)llrint(ldexp((double)wt, RANGE_SHIFT));
  if (q) atomicAdd(row, q);                           // result unused: the no-return form
}

__global__ __launch_bounds__(256) void occ_range_splat(int n, int pair_stride, RangeMulti m,
                                                       unsigned long long* __restrict__ acc) {
  const int64_t total = m.beg[m.levels];
  for (int64_t gp = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; gp < total;
       gp += (int64_t)gridDim.x * blockDim.x) {
    const int l = level_of(m, gp);
    const int h = m.h[l], w = m.w[l];
    const int64_t p = gp - m.beg[l];
    const int j = (int)(p % w);
    const int64_t t2 = p / w;
    const int i = (int)(t2 % h);
    const int s = (int)(t2 / h);                      // the source image: its partner receives
    const float2 g = *reinterpret_cast<const float2*>(m.flow[l] + 2 * p);
    const float x = (float)j + g.x, y = (float)i + g.y;
    const float xf = floorf(x), yf = floorf(y);
    // x0 = floor(x) in [-1, w-1] keeps at least one column in the frame; the test is made on
    // the float, before any conversion, and fails for NaN and +-inf
    if (!(xf >= -1.f && xf <= (float)(w - 1) && yf >= -1.f && yf <= (float)(h - 1))) continue;
    const int x0 = (int)xf, y0 = (int)yf;
    const float fx = x - xf, fy = y - yf;
    const float wx0 = 1.f - fx, wy0 = 1.f - fy;
    // (the integer tests again: past 2^24 the float (w - 1) may have rounded up)
    const bool cx0 = (unsigned)x0 < (unsigned)w, cx1 = (unsigned)(x0 + 1) < (unsigned)w;
    const bool cy0 = (unsigned)y0 < (unsigned)h, cy1 = (unsigned)(y0 + 1) < (unsigned)h;
    unsigned long long* d = acc + m.beg[l] + (int64_t)((s + pair_stride) % n) * h * w +
                            (int64_t)y0 * w + x0;
    range_tap(d, cy0 && cx0, wy0 * wx0);
    range_tap(d + 1, cy0 && cx1, wy0 * fx);
    range_tap(d + w, cy1 && cx0, fy * wx0);
    range_tap(d + w + 1, cy1 && cx1, fy * fx);
  }
}

__global__ __launch_bounds__(256) void occ_range_finish(
    RangeMulti m, const unsigned long long* __restrict__ acc) {
  const int64_t total = m.beg[m.levels];
  for (int64_t gp = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; gp < total;
       gp += (int64_t)gridDim.x * blockDim.x) {
    const int l = level_of(m, gp);
    const int h = m.h[l], w = m.w[l];
    const int64_t p = gp - m.beg[l];
    const float r = (float)ldexp((double)acc[gp], -RANGE_SHIFT);
    if (m.range[l]) m.range[l][p] = r;
    if (m.mask[l]) {
      const int j = (int)(p % w);
      const int i = (int)((p / w) % h);
      const float2 f = *reinterpret_cast<const float2*>(m.flow[l] + 2 * p);
      // occ_mask_multi's border test
      const float x = (float)j + f.x, y = (float)i + f.y;
      const bool ok = x >= 0.f && x <= (float)(w - 1) && y >= 0.f && y <= (float)(h - 1);
      m.mask[l][p] = (ok ? 1.f : 0.f) * fminf(1.f, r);
    }
  }
}

// Pixels of all levels, or -1 for arguments of_occ_range_multi rejects.
static int64_t range_pixels(int n, const int* hs, const int* ws, int levels) {
  if (levels < 1 || levels > 8 || !hs || !ws || n < 2) return -1;
  int64_t total = 0;
  for (int l = 0; l < levels; ++l) {
    if (hs[l] < 1 || ws[l] < 1) return -1;
    const int64_t px = (int64_t)n * hs[l] * ws[l];
    if (px >= (1LL << 40)) return -1;
    total += px;
  }
  return total;
}

}  // namespace oflow

using namespace oflow;

extern "C" {

size_t of_occ_range_ws_bytes(int n, const int* hs, const int* ws, int levels) {
  const int64_t total = range_pixels(n, hs, ws, levels);
  return total < 0 ? 0 : (size_t)total * sizeof(unsigned long long);
}

int of_occ_range_multi(const float* const* flows, int n, int pair_stride, const int* hs,
                       const int* ws, int levels, void* workspace, size_t workspace_bytes,
                       float* const* ranges, float* const* masks, void* stream) {
  static const std::string fn = "of_occ_range_multi";
  RangeMulti m{};
  int st = levels_init(fn, n, hs, ws, levels, m);
  if (st) return st;
  if (!flows) return fail(OF_EINVAL, fn + ": NULL argument");
  if (n < 2 || pair_stride < 1 || (int64_t)n != 2 * (int64_t)pair_stride)
    return fail(OF_EINVAL, fn + ": needs n == 2 * pair_stride, n >= 2");
  if ((st = levels_ptrs8(fn, flows, levels, "flow"))) return st;
  levels_by_pixels(fn, n, m);
  bool any = false;
  for (int l = 0; l < levels; ++l) {
    m.flow[l] = flows[l];
    m.range[l] = ranges ? ranges[l] : nullptr;
    m.mask[l] = masks ? masks[l] : nullptr;
    any = any || m.range[l] || m.mask[l];
  }
  if (!workspace || ((uintptr_t)workspace & 7))
    return fail(OF_EINVAL, fn + ": NULL or not 8-byte aligned workspace");
  if (workspace_bytes < of_occ_range_ws_bytes(n, hs, ws, levels))
    return fail(OF_EINVAL, fn + ": workspace smaller than of_occ_range_ws_bytes");
  if (!any) return fail(OF_EINVAL, fn + ": no output: ranges and masks are both NULL");
  unsigned long long* acc = static_cast<unsigned long long*>(workspace);
  const int64_t total = m.beg[levels];
  const int grid = grid_for(total);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(occ_range_zero, dim3(grid), dim3(256), 0, s, acc, total);
  hipLaunchKernelGGL(occ_range_splat, dim3(grid), dim3(256), 0, s, n, pair_stride, m, acc);
  hipLaunchKernelGGL(occ_range_finish, dim3(grid), dim3(256), 0, s, m, acc);
  return check_launch("occ_range_multi");
}

}  // extern "C"
