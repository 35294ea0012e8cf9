// Structural-similarity (SSIM) data term, 3 x 3 box windows, every pyramid level in one launch.
//   x = image 1, y = warp(image 2, flow) (warp_tap(): the photometric term's sampling), both
//   as intensities I = stored value + channel mean; per channel and per interior centre p
//   (1 <= i <= h-2, 1 <= j <= w-2: windows that stay inside the image)
//   mx, my = 3x3 means,  sx, sy, sxy = 3x3 means of the centred products,
//   S = (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sx + sy + C2)),  d = (1 - S)/2,
//   SSIM_l = sum_p m[p] sum_c d[p,c]      (m: the centre's pixel weight, 1 if none).
// |2 mx my| <= mx^2 + my^2 and |2 sxy| <= sx + sy, so S is in [-1,1] and d in [0,1]: no clamp.
// A workgroup owns an 8 x 32 pixel tile of one image.  Phase 1 stages x and y of the tile plus
// a 2-pixel halo in LDS (the halo's warp is recomputed, no workspace) and keeps the tile
// pixel's dy/d(flow) in registers.  Phase 2: one thread per centre-channel of the tile plus
// 1 pixel forms mu, the centred sums and d; centres inside the tile add m*d to the partial
// (each interior centre lies in exactly one tile), and every centre writes the three
// coefficients of  d d_p/d y_q = a_p + b_p y_q + c_p x_q  (q in p's window) to LDS, 0 where it
// is not interior.  Phase 3: each tile pixel box-sums the coefficients of its up to nine
// windows and writes d SSIM_l / d(flow) as a dense plane, zeros included.  One partial per
// workgroup (wave shuffles, then LDS), no atomics: run-to-run bitwise equal.  The plane is
// scaled into d(flow) by plane_scale_multi (loss_levels.h).
//
// Numerics: LDS holds x and y relative to a per-tile, per-channel reference (the stored values
// of the tile's first pixel), so that the window means and the affine gradient form work on
// small numbers in a low-texture tile, and 1 - S is formed as (1 - lum) + lum (1 - con) with
// 1 - lum = (mx-my)^2 / (mx^2+my^2+C1),  1 - con = mean((x-mx - (y-my))^2) / (sx+sy+C2):
// the same number as the definition's, without the cancellation near S = 1.
#include <algorithm>

#include "loss_levels.h"
#include "warp_tap.h"

namespace oflow {

constexpr int SS_TY = 8, SS_TX = 32, SS_THREADS = SS_TY * SS_TX;
constexpr int SS_SW = SS_TX + 4, SS_SH = SS_TY + 4;      // staged pixels: tile + 2
constexpr int SS_CW = SS_TX + 2, SS_CH = SS_TY + 2;      // centres: tile + 1
constexpr int SS_HALO = SS_SW * SS_SH - SS_THREADS;      // 176 halo pixels
constexpr float SS_C1 = 0.01f * 0.01f, SS_C2 = 0.03f * 0.03f;
static_assert(SS_HALO <= SS_THREADS, "one halo pixel per thread");

// Level l's workgroups are [beg[l], beg[l+1]): one tile and one partial each.
struct SsimMulti : LevelTable {
  const float* img6[8];
  const float* flow[8];
  const float* wt[8];       // (n,h,w) centre weights; NULL: 1
  float* dsdf[8];           // the plane written (all NULL: value only)
  float coef[8];
};

__device__ __forceinline__ float ssim_mean(int c) {
  return c == 0 ? 123.f / 255.f : c == 1 ? 117.f / 255.f : 104.f / 255.f;
}

// x - rx, y - ry and dy/d(flow) (3 channels each) of pixel (i, j) of the image starting at
// pixel offset img.  The bilinear weights sum to 1: blending v - ry is warp(v) - ry.
template <int CV>
__device__ __forceinline__ void ssim_sample(const float* __restrict__ img6,
                                            const float* __restrict__ flow, int i, int j, int h,
                                            int w, int64_t img, const float* rx, const float* ry,
                                            float* xv, float* yv, float* dfx, float* dfy) {
  const int64_t p = img + (int64_t)i * w + j;
  const float2 f = *reinterpret_cast<const float2*>(flow + 2 * p);
  const WarpTap t = warp_tap<CV>(i, j, f.x, f.y, h, w, img);
  const float a = t.a, b = t.b;
  const float w00 = a * b, w01 = a * (1.f - b), w10 = (1.f - a) * b,
              w11 = (1.f - a) * (1.f - b);
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const float v0 = img6[t.o00 * 6 + 3 + e] - ry[e], v1 = img6[t.o01 * 6 + 3 + e] - ry[e];
    const float v2 = img6[t.o10 * 6 + 3 + e] - ry[e], v3 = img6[t.o11 * 6 + 3 + e] - ry[e];
    xv[e] = img6[p * 6 + e] - rx[e];
    yv[e] = w00 * v0 + w01 * v1 + w10 * v2 + w11 * v3;
    // d warped / d flow: the corner differences of photo_l1_bwd_multi (a = x1 - x, b = y1 - y)
    dfx[e] = -(b * (v0 - v2) + (1.f - b) * (v1 - v3));
    dfy[e] = -(a * (v0 - v1) + (1.f - a) * (v2 - v3));
  }
}

// WT: centre weights are read (a template parameter so that the unweighted form loads none).
template <int CV, bool WT>
__global__ __launch_bounds__(SS_THREADS) void ssim_fwd_multi(SsimMulti m,
                                                             float* __restrict__ partials) {
  // planes per channel, rows of 36 / 34 floats: a 32-lane group reads consecutive floats
  // (ds_read_b32 banks are 32 dwords wide), two of them doubled where it crosses a row end
  __shared__ float s_x[3][SS_SH * SS_SW];     // x - rx; 0 outside the image (never read)
  __shared__ float s_y[3][SS_SH * SS_SW];     // y - ry
  __shared__ float s_k[9][SS_CH * SS_CW];     // per centre and channel c: a, b, c at 3c + 0..2
  __shared__ float s_ref[6];                  // rx, ry

  // The level search and the tile decode are spelled out here, not taken from loss_levels.h:
  // through level_of() or tile_of() the compiler fuses and pairs the unpinned products of
  // ssim_sample and of phase 3 differently, and the term and its planes move by an ulp.
  int l = 0;
  while (l + 1 < m.levels && (int64_t)blockIdx.x >= m.beg[l + 1]) ++l;
  const int h = m.h[l], w = m.w[l];
  const float* img6 = m.img6[l];
  const float* flow = m.flow[l];
  int t = (int)((int64_t)blockIdx.x - m.beg[l]);
  const int tcol = t % m.tx[l];
  t /= m.tx[l];
  const int trow = t % m.ty[l];
  const int64_t img = (int64_t)(t / m.ty[l]) * h * w;
  const int y0 = trow * SS_TY, x0 = tcol * SS_TX;
  const int tid = threadIdx.x;
  const int ly = tid / SS_TX, lx = tid % SS_TX;
  const bool grad = m.dsdf[l] != nullptr;

  // ---- phase 1: stage the tile plus 2 pixels ------------------------------------------
  const int64_t p0 = img + (int64_t)y0 * w + x0;      // the tile's first pixel: in the image
  float rx[3], ry[3];
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    rx[e] = img6[p0 * 6 + e];
    ry[e] = img6[p0 * 6 + 3 + e];
  }
  if (tid < 6) s_ref[tid] = img6[p0 * 6 + tid];
  float dfx[3] = {0.f, 0.f, 0.f}, dfy[3] = {0.f, 0.f, 0.f};
  const bool live = y0 + ly < h && x0 + lx < w;
  const int own = (ly + 2) * SS_SW + lx + 2;
  {
    float xv[3] = {0.f, 0.f, 0.f}, yv[3] = {0.f, 0.f, 0.f};
    if (live) ssim_sample<CV>(img6, flow, y0 + ly, x0 + lx, h, w, img, rx, ry, xv, yv, dfx, dfy);
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      s_x[e][own] = xv[e];
      s_y[e][own] = yv[e];
    }
  }
  if (tid < SS_HALO) {
    int hy, hx;      // rows 0, 1, then rows 10, 11, then columns 0, 1, 34, 35 of rows 2..9
    if (tid < 2 * SS_SW) {
      hy = tid / SS_SW;
      hx = tid % SS_SW;
    } else if (tid < 4 * SS_SW) {
      hy = SS_TY + 2 + (tid - 2 * SS_SW) / SS_SW;
      hx = (tid - 2 * SS_SW) % SS_SW;
    } else {
      const int u = tid - 4 * SS_SW;
      hy = 2 + u / 4;
      hx = (u % 4) < 2 ? (u % 4) : SS_TX + (u % 4);
    }
    const int y = y0 - 2 + hy, x = x0 - 2 + hx;
    float xv[3] = {0.f, 0.f, 0.f}, yv[3] = {0.f, 0.f, 0.f}, ux[3], uy[3];
    if (y >= 0 && y < h && x >= 0 && x < w)
      ssim_sample<CV>(img6, flow, y, x, h, w, img, rx, ry, xv, yv, ux, uy);
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      s_x[e][hy * SS_SW + hx] = xv[e];
      s_y[e][hy * SS_SW + hx] = yv[e];
    }
  }
  __syncthreads();

  // ---- phase 2: one thread per centre-channel of the tile plus 1 pixel ------------------
  float s = 0.f;
  for (int k = tid; k < 3 * SS_CH * SS_CW; k += SS_THREADS) {
    const int c = k / (SS_CH * SS_CW), r = k % (SS_CH * SS_CW);
    const int cyl = r / SS_CW, cxl = r % SS_CW;
    const int cy = y0 - 1 + cyl, cx = x0 - 1 + cxl;
    float ka = 0.f, kb = 0.f, kc = 0.f;
    // an interior centre's window lies inside the image, and inside the staged pixels
    if (cy >= 1 && cy <= h - 2 && cx >= 1 && cx <= w - 2) {
      // No contraction in this block: which products the compiler fuses into a following add
      // depends on how often a value is used, and that differs between the weighted and the
      // unweighted instantiation; rounded one by one, weights of 1 give bitwise the
      // unweighted result.
#pragma clang fp contract(off)
      const float* px = s_x[c] + cyl * SS_SW + cxl;      // the window's first pixel
      const float* py = s_y[c] + cyl * SS_SW + cxl;
      float xs[9], ys[9];
      float sx = 0.f, sy = 0.f;
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        xs[q] = px[(q / 3) * SS_SW + q % 3];
        ys[q] = py[(q / 3) * SS_SW + q % 3];
        sx += xs[q];
        sy += ys[q];
      }
      const float mxr = sx * (1.f / 9.f), myr = sy * (1.f / 9.f);   // relative to rx, ry
      float s2 = 0.f, se = 0.f;
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        const float ex = xs[q] - mxr, ey = ys[q] - myr;
        s2 += ex * ex + ey * ey;
        se += (ex - ey) * (ex - ey);
      }
      const float refx = s_ref[c], refy = s_ref[3 + c], mean = ssim_mean(c);
      const float mux = mxr + (refx + mean), muy = myr + (refy + mean);
      const float dm = (mxr - myr) + (refx - refy);                 // mx - my
      const float il = 1.f / (mux * mux + muy * muy + SS_C1);
      const float ic = 1.f / (s2 * (1.f / 9.f) + SS_C2);
      const float oml = dm * dm * il, omc = se * (1.f / 9.f) * ic;   // 1 - lum, 1 - con
      const float lum = 1.f - oml, con = 1.f - omc;
      const float d = 0.5f * (oml + lum * omc);
      float wc = 1.f;
      if (WT) wc = m.wt[l] ? m.wt[l][img + (int64_t)cy * w + cx] : 1.f;
      if (cyl >= 1 && cyl <= SS_TY && cxl >= 1 && cxl <= SS_TX) s += WT ? wc * d : d;
      // P = dd/dmy, Q = 2 dd/dsy, R = dd/dsxy
      const float P = -con * dm * (mux * (mux + muy) + SS_C1) * il * il;
      const float Q = lum * con * ic, R = -lum * ic;
      ka = (P - Q * myr - R * mxr) * (1.f / 9.f);
      kb = Q * (1.f / 9.f);
      kc = R * (1.f / 9.f);
      if (WT) ka *= wc, kb *= wc, kc *= wc;
    }
    if (grad) {
      s_k[3 * c][r] = ka;
      s_k[3 * c + 1][r] = kb;
      s_k[3 * c + 2][r] = kc;
    }
  }

  // ---- phase 3: the tile's pixels gather their windows' coefficients --------------------
  if (grad) {
    __syncthreads();
    if (live) {
      float gx = 0.f, gy = 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float A = 0.f, B = 0.f, Cc = 0.f;
#pragma unroll
        for (int q = 0; q < 9; ++q) {
          const int o = (ly + q / 3) * SS_CW + lx + q % 3;
          A += s_k[3 * c][o];
          B += s_k[3 * c + 1][o];
          Cc += s_k[3 * c + 2][o];
        }
        const float g = A + s_y[c][own] * B + s_x[c][own] * Cc;     // d SSIM_l / d y[q,c]
        gx += g * dfx[c];
        gy += g * dfy[c];
      }
      *reinterpret_cast<float2*>(m.dsdf[l] + 2 * (img + (int64_t)(y0 + ly) * w + x0 + lx)) =
          make_float2(gx, gy);
    }
  }
  const float tot = block_sum_fixed<SS_THREADS>(s);
  if (tid == 0) partials[blockIdx.x] = tot * m.coef[l];
}

}  // namespace oflow

using namespace oflow;

extern "C" {

int of_ssim_partials(int n, int h, int w) {
  if (n < 1 || h < 1 || w < 1) return 0;
  return (int)std::min<int64_t>(n * cdiv(h, SS_TY) * cdiv(w, SS_TX), INT32_MAX);
}

int of_ssim_fwd_multi(const float* const* img6s, const float* const* flows,
                      const float* const* weights, int n, const int* hs, const int* ws,
                      int levels, const float* coefs, float* const* dsdfs, float* partials,
                      int convention, void* stream) {
  static const std::string fn = "of_ssim_fwd_multi";
  if (convention != OF_WARP_REFERENCE && convention != OF_WARP_IMAGE)
    return fail(OF_EINVAL, fn + ": unknown warp convention");
  SsimMulti m{};
  int st = levels_init(fn, n, hs, ws, levels, m);
  if (st) return st;
  if (!img6s || !flows || !coefs) return fail(OF_EINVAL, fn + ": NULL argument");
  if (!partials) return fail(OF_EINVAL, fn + ": NULL partials");
  if ((st = levels_ptrs8(fn, flows, levels, "flow"))) return st;
  if (dsdfs && (st = levels_ptrs8(fn, dsdfs, levels, "dsdf"))) return st;
  bool weighted = false;          // a NULL array or only NULL entries: the unweighted kernel
  for (int l = 0; l < levels; ++l) {
    if (!img6s[l]) return fail(OF_EINVAL, fn + ": NULL image level");
    m.img6[l] = img6s[l];
    m.flow[l] = flows[l];
    m.wt[l] = weights ? weights[l] : nullptr;
    weighted = weighted || m.wt[l];
    m.dsdf[l] = dsdfs ? dsdfs[l] : nullptr;
    m.coef[l] = coefs[l];
  }
  if ((st = levels_by_tiles(fn, n, m, SS_TY, SS_TX))) return st;
  const dim3 grid((unsigned)m.beg[levels]), block(SS_THREADS);
  const bool im = convention == OF_WARP_IMAGE;
  auto k = weighted ? (im ? ssim_fwd_multi<WARP_CV_IMAGE, true> : ssim_fwd_multi<WARP_CV_REFERENCE, true>)
                    : (im ? ssim_fwd_multi<WARP_CV_IMAGE, false> : ssim_fwd_multi<WARP_CV_REFERENCE, false>);
  hipLaunchKernelGGL(k, grid, block, 0, as_stream(stream), m, partials);
  return check_launch("ssim_fwd_multi");
}

int of_ssim_bwd_multi(const float* const* dsdfs, int n, const int* hs, const int* ws, int levels,
                      const float* coefs, const float* dloss, float* const* dflows,
                      const int* lds, int accumulate, void* stream) {
  return plane_scale_multi("of_ssim_bwd_multi", dsdfs, n, hs, ws, levels, coefs, dloss, dflows,
                           lds, accumulate, stream);
}

}  // extern "C"
