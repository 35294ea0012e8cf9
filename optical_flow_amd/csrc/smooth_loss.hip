// Edge-aware first-order flow smoothness (Charbonnier penalty on the flow's first differences,
// weighted by exp(-alpha * mean|d image1|) across the same pixel pair), every pyramid level in
// one launch.  Same shape as the photo_l1_*_multi pair (flow_ops.hip): the forward writes one
// partial per block for of_sum_partials, the backward is a gather (each pixel sums the
// derivative of its four edges), so neither uses atomics and both are run-to-run bitwise equal.
#include <algorithm>

#include "common.h"

namespace oflow {

constexpr int SL_THREADS = 256;
constexpr int SL_PIX_PER_BLOCK = 1024;

// Level l's blocks are [beg[l], beg[l+1]) in the forward (one partial per block, the partial
// arrays concatenated in level order), its pixels [beg[l], beg[l+1]) in the backward.
struct SmoothMulti {
  const float* img6[8];     // all NULL when edge_alpha == 0 (no image byte is read)
  const float* flow[8];
  float* dflow[8];
  int ld[8];
  float cv[8], ch[8];
  int h[8], w[8];
  int64_t beg[9];
  int levels;
};

// Weight of the edge between pixels p and q (image 1 = channels 0..2 of the 6-channel pair).
// Forward and backward both call this, so the gradient is the gradient of the value computed.
__device__ __forceinline__ float edge_weight(const float* __restrict__ img6, int64_t p, int64_t q,
                                             float alpha) {
  const float* a = img6 + p * 6;
  const float* b = img6 + q * 6;
  const float m = (fabsf(a[0] - b[0]) + fabsf(a[1] - b[1]) + fabsf(a[2] - b[2])) * (1.f / 3.f);
  return __expf(-alpha * m);
}

__device__ __forceinline__ float2 flow_at(const float* __restrict__ flow, int64_t p) {
  return *reinterpret_cast<const float2*>(flow + 2 * p);
}

// rho(d) = sqrt(d^2 + eps) over both channels of one edge
__device__ __forceinline__ float edge_rho(float2 a, float2 b, float eps) {
  const float dx = a.x - b.x, dy = a.y - b.y;
  return sqrtf(dx * dx + eps) + sqrtf(dy * dy + eps);
}

// rho'(d) = d / sqrt(d^2 + eps) per channel, d = a - b
__device__ __forceinline__ float2 edge_drho(float2 a, float2 b, float eps) {
  const float dx = a.x - b.x, dy = a.y - b.y;
  return make_float2(dx * rsqrtf(dx * dx + eps), dy * rsqrtf(dy * dy + eps));
}

template <bool EDGE>
__global__ __launch_bounds__(SL_THREADS) void flow_smooth_fwd_multi(int n, SmoothMulti m,
                                                                    float alpha, float eps,
                                                                    float* __restrict__ partials) {
  int l = 0;
  while (l + 1 < m.levels && (int64_t)blockIdx.x >= m.beg[l + 1]) ++l;
  const int h = m.h[l], w = m.w[l];
  const float* img6 = m.img6[l];
  const float* flow = m.flow[l];
  const float cv = m.cv[l], ch = m.ch[l];
  const int64_t npix = (int64_t)n * h * w;
  const int64_t p0 = ((int64_t)blockIdx.x - m.beg[l]) * SL_PIX_PER_BLOCK;
  float s = 0.f;
  for (int k = threadIdx.x; k < SL_PIX_PER_BLOCK; k += SL_THREADS) {
    const int64_t p = p0 + k;
    if (p >= npix) break;
    const int j = (int)(p % w);
    const int i = (int)((p / w) % h);
    const float2 f = flow_at(flow, p);
    if (i + 1 < h) {        // "down" edge: p + w is the same column of the next row, same image
      float r = cv * edge_rho(f, flow_at(flow, p + w), eps);
      if (EDGE) r *= edge_weight(img6, p, p + w, alpha);
      s += r;
    }
    if (j + 1 < w) {        // "right" edge: never across a row end
      float r = ch * edge_rho(f, flow_at(flow, p + 1), eps);
      if (EDGE) r *= edge_weight(img6, p, p + 1, alpha);
      s += r;
    }
  }
  // block reduction in a fixed order: wave shuffles then LDS
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  __shared__ float red[SL_THREADS / 64];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int k = 0; k < SL_THREADS / 64; ++k) t += red[k];
    partials[blockIdx.x] = t;
  }
}

template <bool EDGE>
__global__ __launch_bounds__(256) void flow_smooth_bwd_multi(int n, SmoothMulti m, float alpha,
                                                             float eps,
                                                             const float* __restrict__ dloss,
                                                             int accumulate) {
  const int64_t total = m.beg[m.levels];
  const float dl = dloss ? dloss[0] : 1.f;
  for (int64_t gp = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; gp < total;
       gp += (int64_t)gridDim.x * blockDim.x) {
    int l = 0;
    while (l + 1 < m.levels && gp >= m.beg[l + 1]) ++l;
    const int h = m.h[l], w = m.w[l];
    const float* img6 = m.img6[l];
    const float* flow = m.flow[l];
    const int64_t p = gp - m.beg[l];
    const int j = (int)(p % w);
    const int i = (int)((p / w) % h);
    const float2 f = flow_at(flow, p);
    float vx = 0.f, vy = 0.f, hx = 0.f, hy = 0.f;
    if (i + 1 < h) {        // down: this pixel is the minuend
      float2 g = edge_drho(f, flow_at(flow, p + w), eps);
      const float wt = EDGE ? edge_weight(img6, p, p + w, alpha) : 1.f;
      vx += wt * g.x, vy += wt * g.y;
    }
    if (i > 0) {            // up: this pixel is the subtrahend of the edge owned by p - w
      float2 g = edge_drho(flow_at(flow, p - w), f, eps);
      const float wt = EDGE ? edge_weight(img6, p - w, p, alpha) : 1.f;
      vx -= wt * g.x, vy -= wt * g.y;
    }
    if (j + 1 < w) {        // right
      float2 g = edge_drho(f, flow_at(flow, p + 1), eps);
      const float wt = EDGE ? edge_weight(img6, p, p + 1, alpha) : 1.f;
      hx += wt * g.x, hy += wt * g.y;
    }
    if (j > 0) {            // left
      float2 g = edge_drho(flow_at(flow, p - 1), f, eps);
      const float wt = EDGE ? edge_weight(img6, p - 1, p, alpha) : 1.f;
      hx -= wt * g.x, hy -= wt * g.y;
    }
    const float cv = m.cv[l] * dl, ch = m.ch[l] * dl;
    float gx = cv * vx + ch * hx, gy = cv * vy + ch * hy;
    float* d = m.dflow[l] + (int64_t)m.ld[l] * p;      // channels 2.. of a padded row: untouched
    if (accumulate) gx += d[0], gy += d[1];
    d[0] = gx;
    d[1] = gy;
  }
}

static int smooth_grid(int64_t work) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(work, 256), 8192));
}

// Argument checks shared by both entry points; fills the per-level table but not beg[].
static int smooth_args(const char* fn, const float* const* img6s, const float* const* flows,
                       int n, const int* hs, const int* ws, int levels, float edge_alpha,
                       float eps, const float* coefs_v, const float* coefs_h, SmoothMulti& m) {
  const std::string f(fn);
  if (levels < 1 || levels > 8) return fail(OF_EINVAL, f + ": levels must be 1..8");
  if (!flows || !hs || !ws || !coefs_v || !coefs_h) return fail(OF_EINVAL, f + ": NULL argument");
  if (n < 1) return fail(OF_EINVAL, f + ": n < 1");
  if (!(eps > 0.f)) return fail(OF_EINVAL, f + ": eps must be > 0");
  if (edge_alpha != 0.f && !img6s)
    return fail(OF_EINVAL, f + ": edge_alpha != 0 needs the image pyramid (img6s is NULL)");
  m.levels = levels;
  for (int l = 0; l < levels; ++l) {
    if (hs[l] < 1 || ws[l] < 1) return fail(OF_EINVAL, f + ": h or w < 1");
    if ((int64_t)n * hs[l] * ws[l] >= (1LL << 40))
      return fail(OF_EINVAL, f + ": a level must hold < 2^40 pixels");
    if (!flows[l] || ((uintptr_t)flows[l] & 7))
      return fail(OF_EINVAL, f + ": NULL or not 8-byte aligned flow");
    if (edge_alpha != 0.f && !img6s[l]) return fail(OF_EINVAL, f + ": NULL image level");
    m.img6[l] = edge_alpha != 0.f ? img6s[l] : nullptr;
    m.flow[l] = flows[l];
    m.h[l] = hs[l];
    m.w[l] = ws[l];
    m.cv[l] = coefs_v[l];
    m.ch[l] = coefs_h[l];
  }
  return OF_OK;
}

}  // namespace oflow

using namespace oflow;

extern "C" {

int of_flow_smooth_partials(int n, int h, int w) {
  if (n < 1 || h < 1 || w < 1) return 0;
  return (int)std::min<int64_t>(cdiv((int64_t)n * h * w, SL_PIX_PER_BLOCK), INT32_MAX);
}

int of_flow_smooth_fwd_multi(const float* const* img6s, const float* const* flows, int n,
                             const int* hs, const int* ws, int levels, float edge_alpha,
                             float eps, const float* coefs_v, const float* coefs_h,
                             float* partials, void* stream) {
  static const char* fn = "of_flow_smooth_fwd_multi";
  SmoothMulti m{};
  const int st = smooth_args(fn, img6s, flows, n, hs, ws, levels, edge_alpha, eps, coefs_v,
                             coefs_h, m);
  if (st) return st;
  if (!partials) return fail(OF_EINVAL, std::string(fn) + ": NULL partials");
  m.beg[0] = 0;
  for (int l = 0; l < levels; ++l)
    m.beg[l + 1] = m.beg[l] + of_flow_smooth_partials(n, hs[l], ws[l]);
  if (m.beg[levels] >= INT32_MAX) return fail(OF_EINVAL, std::string(fn) + ": too many blocks");
  const dim3 grid((unsigned)m.beg[levels]), block(SL_THREADS);
  if (edge_alpha != 0.f)
    hipLaunchKernelGGL(flow_smooth_fwd_multi<true>, grid, block, 0, as_stream(stream), n, m,
                       edge_alpha, eps, partials);
  else
    hipLaunchKernelGGL(flow_smooth_fwd_multi<false>, grid, block, 0, as_stream(stream), n, m,
                       edge_alpha, eps, partials);
  return check_launch("flow_smooth_fwd_multi");
}

int of_flow_smooth_bwd_multi(const float* const* img6s, const float* const* flows, int n,
                             const int* hs, const int* ws, int levels, float edge_alpha,
                             float eps, const float* coefs_v, const float* coefs_h,
                             const float* dloss, float* const* dflows, const int* lds,
                             int accumulate, void* stream) {
  static const char* fn = "of_flow_smooth_bwd_multi";
  SmoothMulti m{};
  const int st = smooth_args(fn, img6s, flows, n, hs, ws, levels, edge_alpha, eps, coefs_v,
                             coefs_h, m);
  if (st) return st;
  if (!dflows || !lds) return fail(OF_EINVAL, std::string(fn) + ": NULL argument");
  m.beg[0] = 0;
  for (int l = 0; l < levels; ++l) {
    if (!dflows[l]) return fail(OF_EINVAL, std::string(fn) + ": NULL dflow");
    if (lds[l] < 2) return fail(OF_EINVAL, std::string(fn) + ": lds[l] must be >= 2");
    m.dflow[l] = dflows[l];
    m.ld[l] = lds[l];
    m.beg[l + 1] = m.beg[l] + (int64_t)n * hs[l] * ws[l];
  }
  const dim3 grid(smooth_grid(m.beg[levels])), block(256);
  if (edge_alpha != 0.f)
    hipLaunchKernelGGL(flow_smooth_bwd_multi<true>, grid, block, 0, as_stream(stream), n, m,
                       edge_alpha, eps, dloss, accumulate);
  else
    hipLaunchKernelGGL(flow_smooth_bwd_multi<false>, grid, block, 0, as_stream(stream), n, m,
                       edge_alpha, eps, dloss, accumulate);
  return check_launch("flow_smooth_bwd_multi");
}

}  // extern "C"
