// Supervised term of the training loss (build-added; the reference trains without labels):
// the Charbonnier end-point error of every level's flow against KITTI 16-bit ground truth, in
// native pixels, and its gradient.  include/oflow.h (of_supervised_fwd_multi) states the
// arithmetic; tests/supervised_ref.py restates it in float64.
//
// Two passes, both stream-ordered, nothing read back:
//   count   the valid pixels of every map (integers; the evaluator's flat 48-byte reads), then
//           one wave turns them into the per-image weight 1 / (n_nonempty * n_valid_i);
//   forward every level in one launch, in gather form: a grid cell walks the native pixels whose
//           bilinear footprint touches it, decodes each, samples u through the evaluator's
//           __device__ sampler (flow_sample.h) from a 3 x 3 flow tile staged in LDS (the cell and
//           its one-cell halo hold every tap of the footprint), and sums rho (the pixels whose
//           top-left tap it is) and its own d rho / d cell.  A pixel's residual is recomputed
//           by each of its up to four cells.  No atomics: a lane adds its pixels in index
//           order (double), a wave reduces by a shuffle tree, the waves of a split cell are
//           added in wave order.
// A cell is owned by one wave (four cells per workgroup) while its footprint is small, by the
// four waves of a workgroup (four interleaved slices) once it holds more than kSplitPixels:
// the footprint is 8 x 8 native pixels for a 96 x 320 grid under a 375 x 1242 map and doubles
// per level.  Lanes take the footprint's pixels in flat row-major order, whatever its size.
// A footprint's rows are short runs of 6-byte pixels, so the map is read sample by sample
// (2-byte loads; byte loads when the map sits at an odd address).
#include <algorithm>
#include <cmath>

#include "flow_sample.h"
#include "loss_levels.h"

using namespace oflow;

namespace {

constexpr int kSupThreads = 256;
constexpr int kSupWaves = kSupThreads / kWave;
constexpr int kSplitPixels = 1024;       // footprints above this are split over the four waves
constexpr int kCntThreads = 256;
constexpr int kCntPxPerWg = 4096;
constexpr int kCntMaxWgs = 256;

// h, w: each level's flow grid; beg[l]: the first workgroup of level l.
struct SupMulti : LevelTable {
  const float* flow[8];
  float* plane[8];        // may be NULL: no gradient wanted
  float coef[8];
  int split[8];           // waves per cell: 1 or kSupWaves
};

int count_partials_per_image(int max_gh, int max_gw) {
  const int64_t px = (int64_t)std::max(max_gh, 1) * std::max(max_gw, 1);
  return (int)std::min<int64_t>(std::max<int64_t>(cdiv(px, kCntPxPerWg), 1), kCntMaxWgs);
}

int level_split(int fh, int fw, int max_gh, int max_gw) {
  const int64_t fy = 2 * (int64_t)cdiv(std::max(max_gh, 1), fh) + 2;
  const int64_t fx = 2 * (int64_t)cdiv(std::max(max_gw, 1), fw) + 2;
  return fy * fx > kSplitPixels ? kSupWaves : 1;
}

int64_t level_blocks(int n, int fh, int fw, int split) {
  return (int64_t)n * cdiv((int64_t)fh * fw, kSupWaves / split);
}

int64_t weights_bytes(int n) { return round_up((int64_t)n * 4, 256); }

// Grid (P, n_gt): workgroup b of image i counts the pixels with B != 0 in its share of the flat
// pixel run (8-pixel groups of three 16-byte loads where the map is 16-byte aligned, as
// flow_eval_kernel reads them; byte by byte otherwise, and for the last h*w % 8 pixels).
__global__ __launch_bounds__(kCntThreads) void sup_count_kernel(const uint8_t* __restrict__ raw,
                                                                int* __restrict__ counts) {
  __shared__ int wcnt[kCntThreads / kWave];
  const int tid = threadIdx.x, b = blockIdx.x, P = gridDim.x, img = blockIdx.y;
  const of_image_desc d = reinterpret_cast<const of_image_desc*>(raw)[img];
  int c = 0;
  if (d.h > 0 && d.w > 0) {
    const uint8_t* map = raw + d.offset;
    const int64_t npix = (int64_t)d.h * d.w;
    const int64_t ngroups = npix / 8;
    const int64_t chunk = (ngroups + P - 1) / P;
    const int64_t g0 = std::min<int64_t>((int64_t)b * chunk, ngroups);
    const int64_t g1 = std::min<int64_t>(g0 + chunk, ngroups);
    if (((uintptr_t)map & 15) == 0) {
      const uint4* m4 = reinterpret_cast<const uint4*>(map);
      for (int64_t g = g0 + tid; g < g1; g += kCntThreads) {
        const uint4 q0 = m4[3 * g], q1 = m4[3 * g + 1], q2 = m4[3 * g + 2];
        const unsigned wd[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w,
                                 q2.x, q2.y, q2.z, q2.w};
#pragma unroll
        for (int j = 0; j < 8; ++j)     // sample 3j+2 of the 24 little-endian uint16 in wd
          c += ((wd[(3 * j + 2) >> 1] >> (16 * ((3 * j + 2) & 1))) & 0xffffu) != 0;
      }
    } else {
      for (int64_t p = 8 * g0 + tid; p < 8 * g1; p += kCntThreads) c += ld16(map, 3 * p + 2) != 0;
    }
    const int64_t pt = 8 * ngroups + tid;             // the scalar tail, tid < npix % 8
    if (b == P - 1 && pt < npix) c += ld16(map, 3 * pt + 2) != 0;
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) c += __shfl_down(c, off, kWave);
  if ((tid & (kWave - 1)) == 0) wcnt[tid / kWave] = c;
  __syncthreads();
  if (tid == 0) {
    int t = wcnt[0];
#pragma unroll
    for (int k = 1; k < kCntThreads / kWave; ++k) t += wcnt[k];
    counts[(int64_t)img * P + b] = t;
  }
}

// One wave: lane t sums the records of images t, t + 64, ... in index order (integers), the
// wave adds up the images that hold a valid pixel, and each lane stores its images' weights
// 1 / (n_nonempty * n_valid_i) (0 for an empty image, and for the images n_gt .. n-1, which
// have no ground truth).  A lane parks its counts in the weight slots it later overwrites.
__global__ __launch_bounds__(kWave) void sup_weight_kernel(const int* __restrict__ counts, int P,
                                                           int n_gt, int n,
                                                           float* __restrict__ weights) {
  int* parked = reinterpret_cast<int*>(weights);
  int nonempty = 0;
  for (int i = threadIdx.x; i < n_gt; i += kWave) {
    int t = 0;
    for (int k = 0; k < P; ++k) t += counts[(int64_t)i * P + k];
    parked[i] = t;
    nonempty += t > 0;
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) nonempty += __shfl_xor(nonempty, off, kWave);
  for (int i = threadIdx.x; i < n; i += kWave) {
    const int t = i < n_gt ? parked[i] : 0;
    weights[i] = t > 0 ? (float)(1.0 / ((double)nonempty * (double)t)) : 0.f;
  }
}

// First index whose floor source coordinate (src_coord's i0) is >= k: i0(i) >= k iff
// (2 i + 1) n >= g (2 k + 1), in exact integers.
__device__ __forceinline__ int first_with_floor(int k, int n, int g) {
  if (k <= 0) return 0;
  if (k >= n) return g;
  const int64_t num = (int64_t)g * (2 * k + 1) - n, den = 2 * (int64_t)n;
  if (num <= 0) return 0;
  return (int)std::min<int64_t>((num + den - 1) / den, g);
}

// One workgroup = kSupWaves / split cells of one image of one level (see the head of the file).
__global__ __launch_bounds__(kSupThreads) void sup_fwd_multi(
    const SupMulti m, int n, int n_gt, const uint8_t* __restrict__ raw,
    const float* __restrict__ weights, float hq, float q, float eps2,
    float* __restrict__ partials) {
  __shared__ float2 s_tile[kSupWaves][9];
  __shared__ double s_red[kSupWaves][3];
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
  const int l = level_of(m, blockIdx.x);
  const int fh = m.h[l], fw = m.w[l], S = m.split[l], cpw = kSupWaves / S;
  const int ncell = fh * fw;
  const int bpi = (ncell + cpw - 1) / cpw;
  const int r = (int)((int64_t)blockIdx.x - m.beg[l]);
  const int img = r / bpi, cb = r - img * bpi;
  const int cell = cb * cpw + wave / S, slice = wave % S;
  const bool live = cell < ncell;
  const int cy = live ? cell / fw : 0, cx = live ? cell - cy * fw : 0;
  const float2* f2 = reinterpret_cast<const float2*>(m.flow[l]) + (int64_t)img * ncell;

  float wimg = 0.f;
  int gh = 0, gw = 0;
  int64_t moff = 0;
  if (img < n_gt) {
    const of_image_desc d = reinterpret_cast<const of_image_desc*>(raw)[img];
    wimg = weights[img];
    gh = d.h;
    gw = d.w;
    moff = d.offset;
  }
  const bool work = live && wimg > 0.f && gh > 0 && gw > 0;
  if (work && lane < 9) {
    const int ty = min(max(cy + lane / 3 - 1, 0), fh - 1);
    const int tx = min(max(cx + lane % 3 - 1, 0), fw - 1);
    s_tile[wave][lane] = f2[(int64_t)ty * fw + tx];
  }
  __syncthreads();

  double srho = 0.0, sgx = 0.0, sgy = 0.0;
  float ku = 0.f, kv = 0.f;
  if (work) {
    const Sampler s(nullptr, fh, fw, gh, gw);
    ku = s.ku;
    kv = s.kv;
    const uint8_t* map = raw + moff;
    const bool even = ((uintptr_t)map & 1) == 0;
    const uint16_t* m16 = reinterpret_cast<const uint16_t*>(map);
    const int xlo = first_with_floor(cx - 1, fw, gw), xhi = first_with_floor(cx + 1, fw, gw);
    const int ylo = first_with_floor(cy - 1, fh, gh), yhi = first_with_floor(cy + 1, fh, gh);
    const int pw = xhi - xlo;
    const int total = pw > 0 && yhi > ylo ? pw * (yhi - ylo) : 0;
    for (int k = slice * kWave + lane; k < total; k += S * kWave) {
      const int ry = k / pw;
      const int y = ylo + ry, x = xlo + (k - ry * pw);
      const int64_t p = (int64_t)y * gw + x;
      unsigned R, G, B;
      if (even) {
        R = m16[3 * p], G = m16[3 * p + 1], B = m16[3 * p + 2];
      } else {
        R = ld16(map, 3 * p), G = ld16(map, 3 * p + 1), B = ld16(map, 3 * p + 2);
      }
      if (B == 0) continue;
      int x0, y0;
      float fx, fy;
      src_coord(x, fw, gw, x0, fx);
      src_coord(y, fh, gh, y0, fy);
      const int ax = x0 - cx + 1, ay = y0 - cy + 1;       // tile column / row of the top-left tap
      if ((unsigned)ax > 1u || (unsigned)ay > 1u) continue;   // (never: the range is exact)
      const int x1 = min(x0 + 1, fw - 1), y1 = min(y0 + 1, fh - 1);
      const int bx = x1 - cx + 1, by = y1 - cy + 1;
      const float2 uv = bilerp_uv(s_tile[wave][3 * ay + ax], s_tile[wave][3 * ay + bx],
                                  s_tile[wave][3 * by + ax], s_tile[wave][3 * by + bx], fx, fy,
                                  ku, kv);
      const float gu = ((float)R - 32768.f) / 64.f, gv = ((float)G - 32768.f) / 64.f;
      const float ex = uv.x - gu, ey = uv.y - gv;
      const float r2 = ex * ex + ey * ey + eps2;
      // r2^(q/2) as exp2f(q/2 log2f(r2)) (about 1e-6 relative for r2 up to 10^5;
      // powf's software path cost a third of the kernel)
      const float rho = q == 1.f ? sqrtf(r2) : exp2f(hq * log2f(r2));
      // this cell's weight in the pixel's interpolation; a clamped axis puts both taps here
      const float wx = (x0 == cx ? 1.f - fx : 0.f) + (x1 == cx ? fx : 0.f);
      const float wy = (y0 == cy ? 1.f - fy : 0.f) + (y1 == cy ? fy : 0.f);
      const float g = wx * wy * (q * rho / r2);
      sgx += (double)(g * ex);
      sgy += (double)(g * ey);
      if (x0 == cx && y0 == cy) srho += (double)rho;
    }
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    srho += __shfl_down(srho, off, kWave);
    sgx += __shfl_down(sgx, off, kWave);
    sgy += __shfl_down(sgy, off, kWave);
  }
  if (lane == 0) {
    s_red[wave][0] = srho;
    s_red[wave][1] = sgx;
    s_red[wave][2] = sgy;
  }
  __syncthreads();
  const double scale = (double)m.coef[l] * (double)wimg;
  if (live && slice == 0 && lane == 0 && m.plane[l]) {
    double gx = s_red[wave][1], gy = s_red[wave][2];
    for (int k = 1; k < S; ++k) {
      gx += s_red[wave + k][1];
      gy += s_red[wave + k][2];
    }
    reinterpret_cast<float2*>(m.plane[l])[(int64_t)img * ncell + cell] =
        make_float2((float)(scale * (double)ku * gx), (float)(scale * (double)kv * gy));
  }
  if (tid == 0) {
    double tot = s_red[0][0];
#pragma unroll
    for (int k = 1; k < kSupWaves; ++k) tot += s_red[k][0];
    partials[blockIdx.x] = (float)(scale * tot);
  }
}

}  // namespace

extern "C" {

int of_supervised_partials(int n, int fh, int fw, int max_gh, int max_gw) {
  if (n < 1 || fh < 1 || fw < 1) return 0;
  return (int)std::min<int64_t>(level_blocks(n, fh, fw, level_split(fh, fw, max_gh, max_gw)),
                                INT32_MAX);
}

int64_t of_supervised_workspace_bytes(int n, int max_gh, int max_gw) {
  if (n < 1) return 0;
  return weights_bytes(n) + (int64_t)n * count_partials_per_image(max_gh, max_gw) * 4;
}

int of_supervised_fwd_multi(const float* const* flows, int n, int n_gt, const int* fhs,
                            const int* fws, int levels, const void* dev_gt_raw,
                            const of_image_desc* host_descs, int64_t gt_bytes, int max_gh,
                            int max_gw, float q, float eps, const float* coefs, void* workspace,
                            int64_t workspace_bytes, float* const* dsdfs, float* partials,
                            void* stream) {
  static const std::string fn = "of_supervised_fwd_multi";
  SupMulti m{};
  if (n < 1 || n > 65535) return fail(OF_EINVAL, fn + ": n outside 1..65535");
  int st = levels_init(fn, n, fhs, fws, levels, m, "flow grid size < 1");
  if (st) return st;
  if (!flows || !coefs || !dev_gt_raw || !workspace || !partials)
    return fail(OF_EINVAL, fn + ": NULL argument");
  if (n_gt < 1 || n_gt > n) return fail(OF_EINVAL, fn + ": n_gt outside 1..n");
  if (!(q > 0.f && q <= 2.f)) return fail(OF_EINVAL, fn + ": q must be in (0, 2]");
  if (!(eps > 0.f) || !std::isfinite(eps)) return fail(OF_EINVAL, fn + ": eps must be > 0");
  if (max_gh < 1 || max_gw < 1) return fail(OF_EINVAL, fn + ": max_gh or max_gw < 1");
  if ((uintptr_t)dev_gt_raw & 15) return fail(OF_EINVAL, fn + ": dev_gt_raw must be 16-byte aligned");
  if (((uintptr_t)workspace & 15) || workspace_bytes < of_supervised_workspace_bytes(n, max_gh, max_gw))
    return fail(OF_EINVAL, fn + ": workspace not 16-byte aligned or smaller than "
                                "of_supervised_workspace_bytes(...)");
  if ((uintptr_t)partials & 3) return fail(OF_EINVAL, fn + ": partials must be 4-byte aligned");
  if ((st = levels_ptrs8(fn, flows, levels, "flow"))) return st;
  if (dsdfs && (st = levels_ptrs8(fn, dsdfs, levels, "plane"))) return st;
  m.beg[0] = 0;       // a level's workgroups depend on its split: no levels_by_*()
  for (int l = 0; l < levels; ++l) {
    if ((int64_t)fhs[l] * fws[l] >= INT32_MAX / 4)
      return fail(OF_EINVAL, fn + ": a level must hold < 2^29 cells per image");
    m.flow[l] = flows[l];
    m.plane[l] = dsdfs ? dsdfs[l] : nullptr;
    m.coef[l] = coefs[l];
    m.split[l] = level_split(fhs[l], fws[l], max_gh, max_gw);
    m.beg[l + 1] = m.beg[l] + level_blocks(n, fhs[l], fws[l], m.split[l]);
  }
  if (m.beg[levels] >= INT32_MAX) return fail(OF_EINVAL, fn + ": too many blocks");
  if (host_descs) {
    const int64_t header = round_up((int64_t)n_gt * (int64_t)sizeof(of_image_desc), 256);
    for (int i = 0; i < n_gt; ++i) {
      const of_image_desc& d = host_descs[i];
      if (d.h <= 0 || d.w <= 0 || (int64_t)d.h * d.w >= INT32_MAX)
        return fail(OF_EINVAL, fn + ": descriptor " + std::to_string(i) + " has size " +
                                   std::to_string(d.h) + " x " + std::to_string(d.w));
      const int64_t bytes = (int64_t)d.h * d.w * 6;
      if (d.offset < header || (gt_bytes > 0 && d.offset > gt_bytes - bytes))
        return fail(OF_EINVAL, fn + ": descriptor " + std::to_string(i) +
                                   " lies outside the ground-truth buffer");
    }
  }
  const uint8_t* raw = static_cast<const uint8_t*>(dev_gt_raw);
  float* weights = static_cast<float*>(workspace);
  int* counts = reinterpret_cast<int*>(static_cast<uint8_t*>(workspace) + weights_bytes(n));
  const int P = count_partials_per_image(max_gh, max_gw);
  hipLaunchKernelGGL(sup_count_kernel, dim3(P, n_gt), dim3(kCntThreads), 0, as_stream(stream),
                     raw, counts);
  if (const int st = check_launch("supervised (count)")) return st;
  hipLaunchKernelGGL(sup_weight_kernel, dim3(1), dim3(kWave), 0, as_stream(stream), counts, P,
                     n_gt, n, weights);
  if (const int st = check_launch("supervised (weights)")) return st;
  hipLaunchKernelGGL(sup_fwd_multi, dim3((unsigned)m.beg[levels]), dim3(kSupThreads), 0,
                     as_stream(stream), m, n, n_gt, raw, weights, 0.5f * q, q, eps * eps,
                     partials);
  return check_launch("supervised_fwd_multi");
}

}  // extern "C"
