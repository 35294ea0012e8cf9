// Soft ternary census data term (illumination-robust), every pyramid level in one launch.
//   g1 = S * mean_c image1,  u = S * mean_c warp(image2, flow)   (warp_tap(): the photometric
//   term's sampling),  tau(d) = d / sqrt(c_t + d^2),  phi(e) = e^2 / (c_d + e^2),
//   e[p,o] = tau(g1[p+o] - g1[p]) - tau(u[p+o] - u[p]) over the (2r+1)^2 - 1 window offsets
//   whose p+o lies in the same image,  C = (1/K) sum_p sum_o phi(e[p,o]).
// Forward: a workgroup owns an 8 x 32 pixel tile of one image, computes g1, u and du/d(flow)
// for the tile plus its r-pixel halo (the halo's warp is recomputed, no workspace) into LDS,
// and runs the window loop from LDS.  Every unordered pair appears twice with the same value
// (tau odd, phi even), so dC/du[q] = (2/K) sum_o phi'(e[q,o]) tau'(u[q+o] - u[q]) needs no
// cross-pixel gather: the same loop forms it, and the kernel writes dC/d(flow) = dC/du *
// du/d(flow) as a dense plane.  One partial per workgroup (wave shuffles, then LDS), no
// atomics: run-to-run bitwise equal.  Backward: pixelwise scale of the plane into d(flow)
// (plane_scale_multi, loss_levels.h).
#include <algorithm>

#include "loss_levels.h"
#include "warp_tap.h"

namespace oflow {

constexpr int CN_TY = 8, CN_TX = 32, CN_THREADS = CN_TY * CN_TX;
constexpr int CN_RMAX = 3;
constexpr float CN_S = 255.f;        // images are u8/255 - mean: c_t on the 8-bit scale
constexpr float CN_CT = 0.81f;       // soft ternary sign
constexpr float CN_CD = 0.1f;        // soft Hamming contribution

// Level l's workgroups are [beg[l], beg[l+1]): one tile and one partial each.
struct CensusMulti : LevelTable {
  const float* img6[8];
  const float* flow[8];
  float* dcdf[8];           // the plane written (all NULL: value only)
  float coef[8];
};

__device__ __forceinline__ float census_mean3(float a, float b, float c) {
  return (a + b + c) * (CN_S / 3.f);
}

// g1, u and du/d(flow) of pixel (i, j) of the image starting at pixel offset img (CV: the
// warp convention, warp_tap.h)
template <int CV>
__device__ __forceinline__ void census_sample(const float* __restrict__ img6,
                                              const float* __restrict__ flow, int i, int j,
                                              int h, int w, int64_t img, float2& gu,
                                              float2& du) {
  const int64_t p = img + (int64_t)i * w + j;
  const float2 f = *reinterpret_cast<const float2*>(flow + 2 * p);
  const WarpTap t = warp_tap<CV>(i, j, f.x, f.y, h, w, img);
  const float a = t.a, b = t.b;
  const float w00 = a * b, w01 = a * (1.f - b), w10 = (1.f - a) * b,
              w11 = (1.f - a) * (1.f - b);
  float wv[3], dx[3], dy[3];
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const float v0 = img6[t.o00 * 6 + 3 + e], v1 = img6[t.o01 * 6 + 3 + e];
    const float v2 = img6[t.o10 * 6 + 3 + e], v3 = img6[t.o11 * 6 + 3 + e];
    wv[e] = w00 * v0 + w01 * v1 + w10 * v2 + w11 * v3;
    // d warped / d flow: the corner differences of photo_l1_bwd_multi (a = x1 - x, b = y1 - y)
    dx[e] = -(b * (v0 - v2) + (1.f - b) * (v1 - v3));
    dy[e] = -(a * (v0 - v1) + (1.f - a) * (v2 - v3));
  }
  gu.x = census_mean3(img6[p * 6], img6[p * 6 + 1], img6[p * 6 + 2]);
  gu.y = census_mean3(wv[0], wv[1], wv[2]);
  du.x = census_mean3(dx[0], dx[1], dx[2]);
  du.y = census_mean3(dy[0], dy[1], dy[2]);
}

// tau(d) = d * rsqrt(c_t + d^2), the product rounded on its own: fused into the subtraction
// that forms e, tau(d1) - tau(d2) would not be exactly 0 for d1 == d2.
__device__ __forceinline__ float census_tau(float d, float r) {
#pragma clang fp contract(off)
  return d * r;
}

// Per-level pixel weights of of_census_fwd_multi_w ((n,h,w) floats; NULL: weight 1).
struct CensusWeights {
  const float* w[8];
};

// WT: the weighted form, C = (1/K) sum_p w[p] sum_o phi(e[p,o]).  A pair {q, q+o} is counted
// once from each end with the same value (tau odd, phi even), now with the weights w[q] and
// w[q+o]: dC/du[q] = (1/K) sum_o (w[q] + w[q+o]) phi'(e[q,o]) tau'(u[q+o] - u[q]), still a
// gather from the tile, which holds w for its halo too.  A template parameter so that the
// unweighted instantiations stay the code they were.
template <int R, int CV, bool WT = false>
__global__ __launch_bounds__(CN_THREADS) void census_fwd_multi(CensusMulti m,
                                                               float* __restrict__ partials,
                                                               CensusWeights wt = {}) {
  constexpr int HW = CN_TX + 2 * R, HH = CN_TY + 2 * R;
  constexpr float INV_K = 1.f / (float)((2 * R + 1) * (2 * R + 1) - 1);
  __shared__ float2 s_gu[HH * HW];      // (g1, u); 0 outside the image (never used: masked)
  __shared__ float2 s_du[HH * HW];      // du/d(flow), read at the tile's own pixels only
  __shared__ float s_w[WT ? HH * HW : 1];   // WT: the weights; 0 outside the image

  const int l = level_of(m, blockIdx.x);
  const int h = m.h[l], w = m.w[l];
  const float* img6 = m.img6[l];
  const float* flow = m.flow[l];
  int64_t img;
  int y0, x0;
  tile_of<CN_TY, CN_TX>(m, l, blockIdx.x, img, y0, x0);

  for (int k = threadIdx.x; k < HH * HW; k += CN_THREADS) {
    const int y = y0 - R + k / HW, x = x0 - R + k % HW;
    float2 gu = make_float2(0.f, 0.f), du = make_float2(0.f, 0.f);
    if (y >= 0 && y < h && x >= 0 && x < w) census_sample<CV>(img6, flow, y, x, h, w, img, gu, du);
    s_gu[k] = gu;
    s_du[k] = du;
    if (WT) {
      float wv = 0.f;
      if (y >= 0 && y < h && x >= 0 && x < w)
        wv = wt.w[l] ? wt.w[l][img + (int64_t)y * w + x] : 1.f;
      s_w[k] = wv;
    }
  }
  __syncthreads();

  const int ly = threadIdx.x / CN_TX, lx = threadIdx.x % CN_TX;
  const int y = y0 + ly, x = x0 + lx;
  const bool live = y < h && x < w;
  const int c = (ly + R) * HW + lx + R;
  const float2 ctr = s_gu[c];
  const float wc = WT ? s_w[c] : 1.f;
  float s = 0.f, g = 0.f;
  // one window row per iteration: unrolled over all (2R+1)^2 taps the compiler holds every
  // LDS read of the window in flight (227 VGPRs at R = 3, 2 waves per SIMD)
#pragma unroll 1
  for (int dy = -R; dy <= R; ++dy) {
    const bool oky = live && y + dy >= 0 && y + dy < h;
#pragma unroll
    for (int dx = -R; dx <= R; ++dx) {
      // the pair stays in this image; o = 0 is no pair (it would add exactly 0: e = 0)
      const bool ok = oky && x + dx >= 0 && x + dx < w && (dy != 0 || dx != 0);
      const float2 nb = s_gu[c + dy * HW + dx];
      const float d1 = nb.x - ctr.x, d2 = nb.y - ctr.y;
      const float r2 = rsqrtf(CN_CT + d2 * d2);
      const float e = census_tau(d1, rsqrtf(CN_CT + d1 * d1)) - census_tau(d2, r2);
      const float e2 = e * e;
      const float inv = __builtin_amdgcn_rcpf(CN_CD + e2);
      // phi(e) and phi'(e) * tau'(d2) = (2 c_d e / (c_d + e^2)^2) * (c_t / (c_t + d2^2)^1.5)
      s += ok ? e2 * inv : 0.f;
      if (WT)
        g += ok ? (wc + s_w[c + dy * HW + dx]) * ((e * inv * inv) * (r2 * r2 * r2)) : 0.f;
      else
        g += ok ? (e * inv * inv) * (r2 * r2 * r2) : 0.f;
    }
  }
  if (WT) s *= wc;      // the centre's weight on its window sum
  if (m.dcdf[l] && live) {
    // unweighted: both ends of a pair give the same term, the 2 of it is in the constant
    const float dcdu = g * (WT ? 2.f * CN_CD * CN_CT * INV_K : 2.f * CN_CD * CN_CT * 2.f * INV_K);
    const float2 du = s_du[c];
    *reinterpret_cast<float2*>(m.dcdf[l] + 2 * (img + (int64_t)y * w + x)) =
        make_float2(dcdu * du.x, dcdu * du.y);
  }
  const float tot = block_sum_fixed<CN_THREADS>(s);
  if (threadIdx.x == 0) partials[blockIdx.x] = tot * (m.coef[l] * INV_K);
}

}  // namespace oflow

using namespace oflow;

extern "C" {

int of_census_partials(int n, int h, int w) {
  if (n < 1 || h < 1 || w < 1) return 0;
  return (int)std::min<int64_t>(n * cdiv(h, CN_TY) * cdiv(w, CN_TX), INT32_MAX);
}

int of_census_workspace_floats(int n, int h, int w) {
  return 0;      // the halo's g1 and u are recomputed in the tile: no prep pass
}

int of_census_fwd_multi(const float* const* img6s, const float* const* flows, int n,
                        const int* hs, const int* ws, int levels, int radius,
                        const float* coefs, float* const* workspaces, float* const* dcdfs,
                        float* partials, void* stream) {
  return of_census_fwd_multi_cv(img6s, flows, n, hs, ws, levels, radius, coefs, workspaces, dcdfs,
                                partials, OF_WARP_REFERENCE, stream);
}

int of_census_fwd_multi_cv(const float* const* img6s, const float* const* flows, int n,
                           const int* hs, const int* ws, int levels, int radius,
                           const float* coefs, float* const* workspaces, float* const* dcdfs,
                           float* partials, int convention, void* stream) {
  return of_census_fwd_multi_w(img6s, flows, nullptr, n, hs, ws, levels, radius, coefs,
                               workspaces, dcdfs, partials, convention, stream);
}

int of_census_fwd_multi_w(const float* const* img6s, const float* const* flows,
                          const float* const* weights, int n, const int* hs, const int* ws,
                          int levels, int radius, const float* coefs, float* const* workspaces,
                          float* const* dcdfs, float* partials, int convention, void* stream) {
  static const std::string fn = "of_census_fwd_multi";
  if (convention != OF_WARP_REFERENCE && convention != OF_WARP_IMAGE)
    return fail(OF_EINVAL, fn + ": unknown warp convention");
  CensusMulti m{};
  int st = levels_init(fn, n, hs, ws, levels, m);
  if (st) return st;
  if (radius < 1 || radius > CN_RMAX) return fail(OF_EINVAL, fn + ": radius must be 1..3");
  if (!img6s || !flows || !coefs) return fail(OF_EINVAL, fn + ": NULL argument");
  if (!partials) return fail(OF_EINVAL, fn + ": NULL partials");
  if ((st = levels_ptrs8(fn, flows, levels, "flow"))) return st;
  if (dcdfs && (st = levels_ptrs8(fn, dcdfs, levels, "dcdf"))) return st;
  for (int l = 0; l < levels; ++l) {
    if (!img6s[l]) return fail(OF_EINVAL, fn + ": NULL image level");
    if (of_census_workspace_floats(n, hs[l], ws[l]) > 0 && (!workspaces || !workspaces[l]))
      return fail(OF_EINVAL, fn + ": NULL workspace");
    m.img6[l] = img6s[l];
    m.flow[l] = flows[l];
    m.dcdf[l] = dcdfs ? dcdfs[l] : nullptr;
    m.coef[l] = coefs[l];
  }
  if ((st = levels_by_tiles(fn, n, m, CN_TY, CN_TX))) return st;
  const dim3 grid((unsigned)m.beg[levels]), block(CN_THREADS);
  const bool im = convention == OF_WARP_IMAGE;
  CensusWeights wt{};
  bool weighted = false;          // a NULL array or only NULL entries: the unweighted kernel
  for (int l = 0; l < levels; ++l) {
    wt.w[l] = weights ? weights[l] : nullptr;
    weighted = weighted || wt.w[l];
  }
  if (weighted) {
    auto kw = radius == 1   ? (im ? census_fwd_multi<1, WARP_CV_IMAGE, true> : census_fwd_multi<1, WARP_CV_REFERENCE, true>)
              : radius == 2 ? (im ? census_fwd_multi<2, WARP_CV_IMAGE, true> : census_fwd_multi<2, WARP_CV_REFERENCE, true>)
                            : (im ? census_fwd_multi<3, WARP_CV_IMAGE, true> : census_fwd_multi<3, WARP_CV_REFERENCE, true>);
    hipLaunchKernelGGL(kw, grid, block, 0, as_stream(stream), m, partials, wt);
    return check_launch("census_fwd_multi_w");
  }
  auto k = radius == 1   ? (im ? census_fwd_multi<1, WARP_CV_IMAGE> : census_fwd_multi<1, WARP_CV_REFERENCE>)
           : radius == 2 ? (im ? census_fwd_multi<2, WARP_CV_IMAGE> : census_fwd_multi<2, WARP_CV_REFERENCE>)
                         : (im ? census_fwd_multi<3, WARP_CV_IMAGE> : census_fwd_multi<3, WARP_CV_REFERENCE>);
  hipLaunchKernelGGL(k, grid, block, 0, as_stream(stream), m, partials, wt);
  return check_launch("census_fwd_multi");
}

int of_census_bwd_multi(const float* const* dcdfs, int n, const int* hs, const int* ws,
                        int levels, const float* coefs, const float* dloss,
                        float* const* dflows, const int* lds, int accumulate, void* stream) {
  return plane_scale_multi("of_census_bwd_multi", dcdfs, n, hs, ws, levels, coefs, dloss, dflows,
                           lds, accumulate, stream);
}

}  // extern "C"
