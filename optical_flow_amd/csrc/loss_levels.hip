// The pixelwise plane scaling shared by the loss terms whose forward writes d(term)/d(flow) as
// a dense plane (loss_levels.h, plane_scale_multi).
#include "loss_levels.h"

namespace oflow {

// Level l's pixels are [beg[l], beg[l+1]).
struct PlaneScale : LevelTable {
  const float* plane[8];
  float* dflow[8];
  int ld[8];
  float coef[8];
};

__global__ __launch_bounds__(256) void plane_scale_kernel(PlaneScale m,
                                                          const float* __restrict__ dloss,
                                                          int accumulate) {
  const int64_t total = m.beg[m.levels];
  const float dl = dloss ? dloss[0] : 1.f;
  for (int64_t gp = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; gp < total;
       gp += (int64_t)gridDim.x * blockDim.x) {
    const int l = level_of(m, gp);
    const int64_t p = gp - m.beg[l];
    const float2 v = *reinterpret_cast<const float2*>(m.plane[l] + 2 * p);
    const float c = m.coef[l] * dl;
    float gx = c * v.x, gy = c * v.y;
    float* d = m.dflow[l] + (int64_t)m.ld[l] * p;      // channels 2.. of a padded row: untouched
    if (accumulate) gx += d[0], gy += d[1];
    d[0] = gx;
    d[1] = gy;
  }
}

int plane_scale_multi(const std::string& f, const float* const* planes, int n, const int* hs,
                      const int* ws, int levels, const float* coefs, const float* dloss,
                      float* const* dflows, const int* lds, int accumulate, void* stream) {
  PlaneScale m{};
  int st = levels_init(f, n, hs, ws, levels, m);
  if (st) return st;
  if (!planes || !coefs || !dflows || !lds) return fail(OF_EINVAL, f + ": NULL argument");
  if ((st = levels_ptrs8(f, planes, levels, "dcdf"))) return st;
  for (int l = 0; l < levels; ++l) {
    if (!dflows[l]) return fail(OF_EINVAL, f + ": NULL dflow");
    if (lds[l] < 2) return fail(OF_EINVAL, f + ": lds[l] must be >= 2");
    m.plane[l] = planes[l];
    m.dflow[l] = dflows[l];
    m.ld[l] = lds[l];
    m.coef[l] = coefs[l];
  }
  levels_by_pixels(f, n, m);
  hipLaunchKernelGGL(plane_scale_kernel, dim3(grid_for(m.beg[levels])), dim3(256), 0,
                     as_stream(stream), m, dloss, accumulate);
  return check_launch("plane_scale_multi");
}

}  // namespace oflow
