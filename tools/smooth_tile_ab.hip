// A/B behind DESIGN.md "Flow smoothness term": the smoothness backward of one level with its
// neighbours served by L2/L1 (the form smooth_loss.hip ships) against a 1-pixel-halo LDS tile
// (8 x 32 pixels per block).  Same arithmetic in both; the outputs are compared bit for bit, then
// the two are timed alternately (device events around 10 launches, 30 rounds, stride-4
// accumulating output as in the train step) at three of the bench's level sizes, with and
// without edge weights.  One JSON line per case.  Stand-alone, not part of liboflow:
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/smooth_tile_ab.hip -o smooth_tile_ab
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

__device__ __forceinline__ float2 drho(float2 a, float2 b, float eps) {
  const float dx = a.x - b.x, dy = a.y - b.y;
  return make_float2(dx * rsqrtf(dx * dx + eps), dy * rsqrtf(dy * dy + eps));
}
__device__ __forceinline__ float ew3(float a0, float a1, float a2, float b0, float b1, float b2, float alpha) {
  const float m = (fabsf(a0 - b0) + fabsf(a1 - b1) + fabsf(a2 - b2)) * (1.f / 3.f);
  return __expf(-alpha * m);
}
__device__ __forceinline__ float ewg(const float* img6, int64_t p, int64_t q, float alpha) {
  const float* a = img6 + p * 6; const float* b = img6 + q * 6;
  return ew3(a[0], a[1], a[2], b[0], b[1], b[2], alpha);
}

template <bool EDGE>
__global__ __launch_bounds__(256) void direct(const float* __restrict__ img6, const float* __restrict__ flow,
                                              int n, int h, int w, float alpha, float eps, float cv, float ch,
                                              float* __restrict__ dflow, int ld, int accumulate) {
  const int64_t total = (int64_t)n * h * w;
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < total; p += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(p % w);
    const int i = (int)((p / w) % h);
    const float2 f = *reinterpret_cast<const float2*>(flow + 2 * p);
    float vx = 0.f, vy = 0.f, hx = 0.f, hy = 0.f;
    if (i + 1 < h) { float2 g = drho(f, *reinterpret_cast<const float2*>(flow + 2 * (p + w)), eps);
      const float wt = EDGE ? ewg(img6, p, p + w, alpha) : 1.f; vx += wt * g.x, vy += wt * g.y; }
    if (i > 0) { float2 g = drho(*reinterpret_cast<const float2*>(flow + 2 * (p - w)), f, eps);
      const float wt = EDGE ? ewg(img6, p - w, p, alpha) : 1.f; vx -= wt * g.x, vy -= wt * g.y; }
    if (j + 1 < w) { float2 g = drho(f, *reinterpret_cast<const float2*>(flow + 2 * (p + 1)), eps);
      const float wt = EDGE ? ewg(img6, p, p + 1, alpha) : 1.f; hx += wt * g.x, hy += wt * g.y; }
    if (j > 0) { float2 g = drho(*reinterpret_cast<const float2*>(flow + 2 * (p - 1)), f, eps);
      const float wt = EDGE ? ewg(img6, p - 1, p, alpha) : 1.f; hx -= wt * g.x, hy -= wt * g.y; }
    float gx = cv * vx + ch * hx, gy = cv * vy + ch * hy;
    float* d = dflow + (int64_t)ld * p;
    if (accumulate) gx += d[0], gy += d[1];
    d[0] = gx; d[1] = gy;
  }
}

constexpr int TR = 8, TC = 32, HR = TR + 2, HC = TC + 2, HN = HR * HC;   // 340 halo entries

template <bool EDGE>
__global__ __launch_bounds__(256) void tiled(const float* __restrict__ img6, const float* __restrict__ flow,
                                             int n, int h, int w, float alpha, float eps, float cv, float ch,
                                             float* __restrict__ dflow, int ld, int accumulate) {
  __shared__ float2 sf[HN];
  __shared__ float si[EDGE ? HN * 3 : 1];
  const int tw = (w + TC - 1) / TC, th = (h + TR - 1) / TR;
  const int bid = blockIdx.x;
  const int b = bid / (tw * th);
  const int i0 = ((bid / tw) % th) * TR, j0 = (bid % tw) * TC;
  if (b >= n) return;
  for (int e = threadIdx.x; e < HN; e += 256) {
    const int gi = i0 + e / HC - 1, gj = j0 + e % HC - 1;
    if (gi >= 0 && gi < h && gj >= 0 && gj < w) {
      const int64_t p = ((int64_t)b * h + gi) * w + gj;
      sf[e] = *reinterpret_cast<const float2*>(flow + 2 * p);
      if (EDGE) { si[3 * e] = img6[p * 6]; si[3 * e + 1] = img6[p * 6 + 1]; si[3 * e + 2] = img6[p * 6 + 2]; }
    }
  }
  __syncthreads();
  const int r = threadIdx.x / TC, c = threadIdx.x % TC;
  const int i = i0 + r, j = j0 + c;
  if (i >= h || j >= w) return;
  const int e = (r + 1) * HC + c + 1;
  const float2 f = sf[e];
  auto wt = [&](int a, int bq) {
    return EDGE ? ew3(si[3 * a], si[3 * a + 1], si[3 * a + 2], si[3 * bq], si[3 * bq + 1], si[3 * bq + 2], alpha) : 1.f;
  };
  float vx = 0.f, vy = 0.f, hx = 0.f, hy = 0.f;
  if (i + 1 < h) { float2 g = drho(f, sf[e + HC], eps); const float t = wt(e, e + HC); vx += t * g.x, vy += t * g.y; }
  if (i > 0) { float2 g = drho(sf[e - HC], f, eps); const float t = wt(e - HC, e); vx -= t * g.x, vy -= t * g.y; }
  if (j + 1 < w) { float2 g = drho(f, sf[e + 1], eps); const float t = wt(e, e + 1); hx += t * g.x, hy += t * g.y; }
  if (j > 0) { float2 g = drho(sf[e - 1], f, eps); const float t = wt(e - 1, e); hx -= t * g.x, hy -= t * g.y; }
  float gx = cv * vx + ch * hx, gy = cv * vy + ch * hy;
  const int64_t p = ((int64_t)b * h + i) * w + j;
  float* d = dflow + (int64_t)ld * p;
  if (accumulate) gx += d[0], gy += d[1];
  d[0] = gx; d[1] = gy;
}

static float median(std::vector<float> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

template <bool EDGE>
static int run(int n, int h, int w, float alpha) {
  const int64_t npix = (int64_t)n * h * w;
  std::vector<float> hf(npix * 2), hi(npix * 6);
  uint32_t s = 12345u;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.f; };
  for (auto& v : hf) v = (rnd() - 0.5f) * 6.f;
  for (auto& v : hi) v = rnd() - 0.5f;
  float *f, *im, *d1, *d2;
  CK(hipMalloc(&f, npix * 8)); CK(hipMalloc(&im, npix * 24)); CK(hipMalloc(&d1, npix * 16)); CK(hipMalloc(&d2, npix * 16));
  CK(hipMemcpy(f, hf.data(), npix * 8, hipMemcpyHostToDevice));
  CK(hipMemcpy(im, hi.data(), npix * 24, hipMemcpyHostToDevice));
  CK(hipMemset(d1, 0, npix * 16)); CK(hipMemset(d2, 0, npix * 16));
  const int gd = (int)std::min<int64_t>((npix + 255) / 256, 8192);
  const int gt = n * ((h + TR - 1) / TR) * ((w + TC - 1) / TC);
  const float eps = 1e-4f, cv = 0.3f, ch = 0.7f;
  // equality: overwrite, stride 4
  hipLaunchKernelGGL(direct<EDGE>, dim3(gd), dim3(256), 0, 0, im, f, n, h, w, alpha, eps, cv, ch, d1, 4, 0);
  hipLaunchKernelGGL(tiled<EDGE>, dim3(gt), dim3(256), 0, 0, im, f, n, h, w, alpha, eps, cv, ch, d2, 4, 0);
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  std::vector<float> o1(npix * 4), o2(npix * 4);
  CK(hipMemcpy(o1.data(), d1, npix * 16, hipMemcpyDeviceToHost));
  CK(hipMemcpy(o2.data(), d2, npix * 16, hipMemcpyDeviceToHost));
  const bool same = memcmp(o1.data(), o2.data(), npix * 16) == 0;
  double nrm = 0; for (auto v : o1) nrm += (double)v * v;
  double maxd = 0; for (size_t k = 0; k < o1.size(); ++k) maxd = std::max(maxd, (double)fabsf(o1[k] - o2[k]));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const int REP = 10, ROUNDS = 30;
  std::vector<float> td, tt;
  for (int r = 0; r < ROUNDS + 3; ++r) {
    for (int v = 0; v < 2; ++v) {
      CK(hipEventRecord(e0, 0));
      for (int k = 0; k < REP; ++k) {
        if (v == 0) hipLaunchKernelGGL(direct<EDGE>, dim3(gd), dim3(256), 0, 0, im, f, n, h, w, alpha, eps, cv, ch, d1, 4, 1);
        else hipLaunchKernelGGL(tiled<EDGE>, dim3(gt), dim3(256), 0, 0, im, f, n, h, w, alpha, eps, cv, ch, d2, 4, 1);
      }
      CK(hipEventRecord(e1, 0));
      CK(hipEventSynchronize(e1));
      float ms; CK(hipEventElapsedTime(&ms, e0, e1));
      if (r >= 3) (v == 0 ? td : tt).push_back(ms * 1000.f / REP);
    }
  }
  CK(hipGetLastError());
  printf("{\"n\": %d, \"h\": %d, \"w\": %d, \"edge_alpha\": %g, \"outputs_bitwise_equal\": %s, \"out_norm\": %.4f, \"max_abs_diff\": %.3g, "
         "\"direct_us_median\": %.2f, \"direct_us_min\": %.2f, \"tiled_us_median\": %.2f, \"tiled_us_min\": %.2f}\n",
         n, h, w, alpha, same ? "true" : "false", sqrt(nrm), maxd, median(td), *std::min_element(td.begin(), td.end()),
         median(tt), *std::min_element(tt.begin(), tt.end()));
  CK(hipFree(f)); CK(hipFree(im)); CK(hipFree(d1)); CK(hipFree(d2));
  return same ? 0 : 1;
}

int main() {
  int rc = 0;
  const int sizes[3][2] = {{192, 256}, {96, 128}, {24, 32}};
  for (auto& sz : sizes) {
    rc |= run<true>(8, sz[0], sz[1], 10.f);
    if (rc & 2) return rc;
    rc |= run<false>(8, sz[0], sz[1], 0.f);
    if (rc & 2) return rc;
  }
  return rc;
}
