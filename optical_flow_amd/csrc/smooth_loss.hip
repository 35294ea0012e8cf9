// Edge-aware first-order flow smoothness (Charbonnier penalty on the flow's first differences,
// weighted by exp(-alpha * mean|d image1|) across the same pixel pair), every pyramid level in
// one launch.  Same shape as the photo_l1_*_multi pair (flow_ops.hip): the forward writes one
// partial per block for of_sum_partials, the backward is a gather (each pixel sums the
// derivative of its four edges), so neither uses atomics and both are run-to-run bitwise equal.
//
// The second-order term (flow_smooth2_*_multi, below) penalises the flow's second differences
// f[p-1] - 2 f[p] + f[p+1] per direction, weighted by the image difference across the triple's
// two outer pixels.  Its stencil is five pixels wide per direction in the backward, so both of
// its kernels stage an 8 x 32 pixel tile plus halo in LDS (the shape of census_loss.hip).
#include <algorithm>

#include "loss_levels.h"

namespace oflow {

constexpr int SL_THREADS = 256;
constexpr int SL_PIX_PER_BLOCK = 1024;

// Level l's blocks are [beg[l], beg[l+1]) in the forward (one partial per block, the partial
// arrays concatenated in level order), its pixels [beg[l], beg[l+1]) in the backward; its tiles
// in both second-order kernels.
struct SmoothMulti : LevelTable {
  const float* img6[8];     // all NULL when edge_alpha == 0 (no image byte is read)
  const float* flow[8];
  float* dflow[8];
  int ld[8];
  float cv[8], ch[8];
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
  const int l = level_of(m, blockIdx.x);
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
  const float t = block_sum_fixed<SL_THREADS>(s);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
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
    const int l = level_of(m, gp);
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

// Argument checks shared by all four entry points; fills the per-level table but not beg[].
static int smooth_args(const char* fn, const float* const* img6s, const float* const* flows,
                       int n, const int* hs, const int* ws, int levels, float edge_alpha,
                       float eps, const float* coefs_v, const float* coefs_h, SmoothMulti& m) {
  const std::string f(fn);
  int st = levels_init(f, n, hs, ws, levels, m);
  if (st) return st;
  if (!flows || !coefs_v || !coefs_h) return fail(OF_EINVAL, f + ": NULL argument");
  if (!(eps > 0.f)) return fail(OF_EINVAL, f + ": eps must be > 0");
  if (edge_alpha != 0.f && !img6s)
    return fail(OF_EINVAL, f + ": edge_alpha != 0 needs the image pyramid (img6s is NULL)");
  if ((st = levels_ptrs8(f, flows, levels, "flow"))) return st;
  for (int l = 0; l < levels; ++l) {
    if (edge_alpha != 0.f && !img6s[l]) return fail(OF_EINVAL, f + ": NULL image level");
    m.img6[l] = edge_alpha != 0.f ? img6s[l] : nullptr;
    m.flow[l] = flows[l];
    m.cv[l] = coefs_v[l];
    m.ch[l] = coefs_h[l];
  }
  return OF_OK;
}

// ---------------------------------------------------------------- second order ----
constexpr int S2_TY = 8, S2_TX = 32, S2_THREADS = S2_TY * S2_TX;

// Second difference of a triple (outer, centre, outer), products rounded on their own so that
// forward and backward form the same value.
__device__ __forceinline__ float2 smooth2_d2(float2 a, float2 b, float2 c) {
#pragma clang fp contract(off)
  return make_float2((a.x - 2.f * b.x) + c.x, (a.y - 2.f * b.y) + c.y);
}

// The halo tile of one workgroup in LDS: flows as float2, image 1 as three planes (EDGE only).
// Positions outside the image hold 0 and are never used: every triple is masked by its
// centre's coordinates.
template <bool EDGE, int HALO>
struct Smooth2Tile {
  static constexpr int HW = S2_TX + 2 * HALO, HH = S2_TY + 2 * HALO, N = HH * HW;
  float2 f[N];
  float i[EDGE ? 3 : 1][EDGE ? N : 1];

  __device__ __forceinline__ void load(const float* __restrict__ img6,
                                       const float* __restrict__ flow, int64_t img, int y0,
                                       int x0, int h, int w) {
    for (int k = threadIdx.x; k < N; k += S2_THREADS) {
      const int y = y0 - HALO + k / HW, x = x0 - HALO + k % HW;
      float2 v = make_float2(0.f, 0.f);
      float a0 = 0.f, a1 = 0.f, a2 = 0.f;
      if (y >= 0 && y < h && x >= 0 && x < w) {
        const int64_t p = img + (int64_t)y * w + x;
        v = flow_at(flow, p);
        if (EDGE) a0 = img6[p * 6], a1 = img6[p * 6 + 1], a2 = img6[p * 6 + 2];
      }
      f[k] = v;
      if (EDGE) i[0][k] = a0, i[1][k] = a1, i[2][k] = a2;
    }
  }

  // weight of the triple whose outer pixels are LDS positions p and q
  __device__ __forceinline__ float weight(int p, int q, float alpha) const {
    if (!EDGE) return 1.f;
    const float m = (fabsf(i[0][p] - i[0][q]) + fabsf(i[1][p] - i[1][q]) +
                     fabsf(i[2][p] - i[2][q])) * (1.f / 3.f);
    return __expf(-alpha * m);
  }
};

template <bool EDGE>
__global__ __launch_bounds__(S2_THREADS) void flow_smooth2_fwd_multi(
    SmoothMulti m, float alpha, float eps, float* __restrict__ partials) {
  using Tile = Smooth2Tile<EDGE, 1>;
  __shared__ Tile s;
  int64_t img;
  int y0, x0;
  const int l = level_of(m, blockIdx.x);
  tile_of<S2_TY, S2_TX>(m, l, blockIdx.x, img, y0, x0);
  const int h = m.h[l], w = m.w[l];
  s.load(m.img6[l], m.flow[l], img, y0, x0, h, w);
  __syncthreads();

  // each pixel of the tile is the centre of (at most) one vertical and one horizontal triple
  const int ly = threadIdx.x / S2_TX, lx = threadIdx.x % S2_TX;
  const int y = y0 + ly, x = x0 + lx;
  const int c = (ly + 1) * Tile::HW + lx + 1;
  float r = 0.f;
  if (y < h && x < w) {
    const float2 f = s.f[c];
    if (y >= 1 && y + 1 < h) {
      const float2 d = smooth2_d2(s.f[c - Tile::HW], f, s.f[c + Tile::HW]);
      r += m.cv[l] * s.weight(c - Tile::HW, c + Tile::HW, alpha) *
           (sqrtf(d.x * d.x + eps) + sqrtf(d.y * d.y + eps));
    }
    if (x >= 1 && x + 1 < w) {      // never across a row end
      const float2 d = smooth2_d2(s.f[c - 1], f, s.f[c + 1]);
      r += m.ch[l] * s.weight(c - 1, c + 1, alpha) *
           (sqrtf(d.x * d.x + eps) + sqrtf(d.y * d.y + eps));
    }
  }
  const float t = block_sum_fixed<S2_THREADS>(r);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// t = w2 * rho'(d2) of one triple, both channels
__device__ __forceinline__ float2 smooth2_t(float2 d, float wt, float eps) {
  return make_float2(wt * d.x * rsqrtf(d.x * d.x + eps), wt * d.y * rsqrtf(d.y * d.y + eps));
}

template <bool EDGE>
__global__ __launch_bounds__(S2_THREADS) void flow_smooth2_bwd_multi(
    SmoothMulti m, float alpha, float eps, const float* __restrict__ dloss, int accumulate) {
  using Tile = Smooth2Tile<EDGE, 2>;
  constexpr int HW = Tile::HW;
  constexpr int NV = (S2_TY + 2) * S2_TX;       // vertical centres: the tile's rows -1 .. TY
  constexpr int TW = S2_TX + 2, NH = S2_TY * TW;    // horizontal ones: its columns -1 .. TX
  __shared__ Tile s;
  __shared__ float2 tv[NV], th[NH];
  int64_t img;
  int y0, x0;
  const int l = level_of(m, blockIdx.x);
  tile_of<S2_TY, S2_TX>(m, l, blockIdx.x, img, y0, x0);
  const int h = m.h[l], w = m.w[l];
  s.load(m.img6[l], m.flow[l], img, y0, x0, h, w);
  __syncthreads();

  // every triple's t once; a centre that has no triple (outside the image, or in its first or
  // last row / column) gets 0, so the gather below needs no case of its own
  for (int k = threadIdx.x; k < NV + NH; k += S2_THREADS) {
    float2 t = make_float2(0.f, 0.f);
    if (k < NV) {
      const int r = k / S2_TX, cc = k % S2_TX;
      const int y = y0 - 1 + r, x = x0 + cc;
      const int c = (r + 1) * HW + cc + 2;
      if (y >= 1 && y + 1 < h && x < w)
        t = smooth2_t(smooth2_d2(s.f[c - HW], s.f[c], s.f[c + HW]),
                      s.weight(c - HW, c + HW, alpha), eps);
      tv[k] = t;
    } else {
      const int r = (k - NV) / TW, cc = (k - NV) % TW;
      const int y = y0 + r, x = x0 - 1 + cc;
      const int c = (r + 2) * HW + cc + 1;
      if (y < h && x >= 1 && x + 1 < w)
        t = smooth2_t(smooth2_d2(s.f[c - 1], s.f[c], s.f[c + 1]), s.weight(c - 1, c + 1, alpha),
                      eps);
      th[k - NV] = t;
    }
  }
  __syncthreads();

  const int ly = threadIdx.x / S2_TX, lx = threadIdx.x % S2_TX;
  const int y = y0 + ly, x = x0 + lx;
  if (y >= h || x >= w) return;
  // this pixel is an outer pixel of the triples centred one step either side, the centre of its own
  const float2 va = tv[ly * S2_TX + lx], vb = tv[(ly + 1) * S2_TX + lx],
               vc = tv[(ly + 2) * S2_TX + lx];
  const float2 ha = th[ly * TW + lx], hb = th[ly * TW + lx + 1], hc = th[ly * TW + lx + 2];
  const float dl = dloss ? dloss[0] : 1.f;
  const float cv = m.cv[l] * dl, ch = m.ch[l] * dl;
  float gx = cv * (va.x - 2.f * vb.x + vc.x) + ch * (ha.x - 2.f * hb.x + hc.x);
  float gy = cv * (va.y - 2.f * vb.y + vc.y) + ch * (ha.y - 2.f * hb.y + hc.y);
  // channels 2.. of a padded row: untouched
  float* d = m.dflow[l] + (int64_t)m.ld[l] * (img + (int64_t)y * w + x);
  if (accumulate) gx += d[0], gy += d[1];
  d[0] = gx;
  d[1] = gy;
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
  if (const int sb = levels_by_pixels(fn, n, m, SL_PIX_PER_BLOCK)) return sb;
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
  for (int l = 0; l < levels; ++l) {
    if (!dflows[l]) return fail(OF_EINVAL, std::string(fn) + ": NULL dflow");
    if (lds[l] < 2) return fail(OF_EINVAL, std::string(fn) + ": lds[l] must be >= 2");
    m.dflow[l] = dflows[l];
    m.ld[l] = lds[l];
  }
  levels_by_pixels(fn, n, m);
  const dim3 grid(grid_for(m.beg[levels])), block(256);
  if (edge_alpha != 0.f)
    hipLaunchKernelGGL(flow_smooth_bwd_multi<true>, grid, block, 0, as_stream(stream), n, m,
                       edge_alpha, eps, dloss, accumulate);
  else
    hipLaunchKernelGGL(flow_smooth_bwd_multi<false>, grid, block, 0, as_stream(stream), n, m,
                       edge_alpha, eps, dloss, accumulate);
  return check_launch("flow_smooth_bwd_multi");
}

int of_flow_smooth2_partials(int n, int h, int w) {
  if (n < 1 || h < 1 || w < 1) return 0;
  return (int)std::min<int64_t>(n * cdiv(h, S2_TY) * cdiv(w, S2_TX), INT32_MAX);
}

int of_flow_smooth2_fwd_multi(const float* const* img6s, const float* const* flows, int n,
                              const int* hs, const int* ws, int levels, float edge_alpha,
                              float eps, const float* coefs_v, const float* coefs_h,
                              float* partials, void* stream) {
  static const char* fn = "of_flow_smooth2_fwd_multi";
  SmoothMulti m{};
  int st = smooth_args(fn, img6s, flows, n, hs, ws, levels, edge_alpha, eps, coefs_v, coefs_h, m);
  if (st) return st;
  if (!partials) return fail(OF_EINVAL, std::string(fn) + ": NULL partials");
  if ((st = levels_by_tiles(fn, n, m, S2_TY, S2_TX))) return st;
  const dim3 grid((unsigned)m.beg[levels]), block(S2_THREADS);
  if (edge_alpha != 0.f)
    hipLaunchKernelGGL(flow_smooth2_fwd_multi<true>, grid, block, 0, as_stream(stream), m,
                       edge_alpha, eps, partials);
  else
    hipLaunchKernelGGL(flow_smooth2_fwd_multi<false>, grid, block, 0, as_stream(stream), m,
                       edge_alpha, eps, partials);
  return check_launch("flow_smooth2_fwd_multi");
}

int of_flow_smooth2_bwd_multi(const float* const* img6s, const float* const* flows, int n,
                              const int* hs, const int* ws, int levels, float edge_alpha,
                              float eps, const float* coefs_v, const float* coefs_h,
                              const float* dloss, float* const* dflows, const int* lds,
                              int accumulate, void* stream) {
  static const char* fn = "of_flow_smooth2_bwd_multi";
  SmoothMulti m{};
  int st = smooth_args(fn, img6s, flows, n, hs, ws, levels, edge_alpha, eps, coefs_v, coefs_h, m);
  if (st) return st;
  if (!dflows || !lds) return fail(OF_EINVAL, std::string(fn) + ": NULL argument");
  for (int l = 0; l < levels; ++l) {
    if (!dflows[l]) return fail(OF_EINVAL, std::string(fn) + ": NULL dflow");
    if (lds[l] < 2) return fail(OF_EINVAL, std::string(fn) + ": lds[l] must be >= 2");
    m.dflow[l] = dflows[l];
    m.ld[l] = lds[l];
  }
  if ((st = levels_by_tiles(fn, n, m, S2_TY, S2_TX))) return st;
  const dim3 grid((unsigned)m.beg[levels]), block(S2_THREADS);
  if (edge_alpha != 0.f)
    hipLaunchKernelGGL(flow_smooth2_bwd_multi<true>, grid, block, 0, as_stream(stream), m,
                       edge_alpha, eps, dloss, accumulate);
  else
    hipLaunchKernelGGL(flow_smooth2_bwd_multi<false>, grid, block, 0, as_stream(stream), m,
                       edge_alpha, eps, dloss, accumulate);
  return check_launch("flow_smooth2_bwd_multi");
}

}  // extern "C"
