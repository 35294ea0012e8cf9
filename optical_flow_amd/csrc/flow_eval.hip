// Evaluation against KITTI 2015 flow ground truth (build-added; the reference has no
// evaluation): mean end-point error and the Fl outlier count of the net's finest
// flow, in one pass over the ground-truth pixels.  Per pixel the flow is upsampled (half-pixel
// centres, border replication), scaled to native pixels, compared with the decoded 16-bit map
// and reduced; the full-resolution flow is never written.  of_flow_upsample writes that
// upsampled flow when it is wanted (predictions, KITTI-format result files) through the same
// __device__ sampler.  include/oflow.h states the arithmetic; tests/kitti_flow_np.py restates
// it in float64.
//
// Traffic: 6 bytes of ground truth per pixel, the flow tile comes through the caches.  A map
// is dense (h x w x 3 uint16, no row padding), so it is read as one flat run of pixels: eight
// pixels are 48 bytes = three 16-byte loads per lane, whatever the width; the last h*w % 8
// pixels and any map whose offset is not 16-byte aligned go byte by byte.  Measured, the
// kernel is bound by the latency of the valid pixels' flow taps, not by bandwidth, and is left
// so: decoding the PNGs takes several hundred times longer (DESIGN.md §3 "Evaluation").
#include <algorithm>
#include <cmath>

#include "common.h"
#include "flow_sample.h"

using namespace oflow;

namespace {

constexpr int kEvalThreads = 256;
constexpr int kEvalWaves = kEvalThreads / kWave;
constexpr int kEvalPxPerWg = 4096;     // pixels per workgroup before P saturates (2 rounds of 8)
constexpr int kEvalMaxWgs = 256;       // partial records per image, at most

struct EvalRec {          // of_flow_eval_result, and one workgroup's partial
  double sum_epe;
  long long n_valid;
  long long n_outlier;
};
static_assert(sizeof(EvalRec) == 24 && sizeof(of_flow_eval_result) == 24,
              "of_flow_eval_result layout is part of the ABI");
static_assert(sizeof(of_image_desc) == 16, "of_image_desc layout is part of the ABI");

int partials_per_image(int max_gh, int max_gw) {
  const int64_t px = (int64_t)std::max(max_gh, 1) * std::max(max_gw, 1);
  return (int)std::min<int64_t>(std::max<int64_t>(cdiv(px, kEvalPxPerWg), 1), kEvalMaxWgs);
}

struct Acc {
  double sum = 0.0;
  int valid = 0, outlier = 0;     // per lane: far below 2^31 pixels
};

// One ground-truth pixel: decode, and when valid sample, compare, count.
__device__ __forceinline__ void eval_pixel(const Sampler& s, int x, int y, unsigned R, unsigned G,
                                           unsigned B, Acc& a) {
  if (B == 0) return;
  const float gu = ((float)R - 32768.f) / 64.f, gv = ((float)G - 32768.f) / 64.f;
  const float2 uv = sample_uv(s, x, y);
  const float du = uv.x - gu, dv = uv.y - gv;
  const float epe = sqrtf(du * du + dv * dv);
  a.sum += (double)epe;
  a.valid += 1;
  if (epe > 3.f && epe > 0.05f * sqrtf(gu * gu + gv * gv)) a.outlier += 1;
}

// Grid (P, n): workgroup b of image i owns the 8-pixel groups [b*chunk, min((b+1)*chunk, G)),
// G = h*w / 8, chunk = ceil(G / P), of the flat pixel run; the last workgroup also the h*w % 8
// pixels after the last group.  Fixed order: a lane sums its pixels in index order, a wave
// reduces by a shuffle tree, thread 0 sums the wave sums in wave order.  One plain record store
// per workgroup; an empty range (or a map with h, w <= 0) stores zeros.
__global__ __launch_bounds__(kEvalThreads) void flow_eval_kernel(
    const float* __restrict__ flow, int fh, int fw, const uint8_t* __restrict__ raw,
    EvalRec* __restrict__ partials) {
  __shared__ double wsum[kEvalWaves];
  __shared__ int wval[kEvalWaves], wout[kEvalWaves];
  const int tid = threadIdx.x, b = blockIdx.x, P = gridDim.x, img = blockIdx.y;
  const of_image_desc d = reinterpret_cast<const of_image_desc*>(raw)[img];
  const int gh = d.h, gw = d.w;
  Acc a;
  if (gh > 0 && gw > 0) {
    const Sampler s(flow + (int64_t)img * fh * fw * 2, fh, fw, gh, gw);
    const uint8_t* map = raw + d.offset;
    const int64_t npix = (int64_t)gh * gw;
    const int64_t ngroups = npix / 8;
    const int64_t chunk = (ngroups + P - 1) / P;
    const int64_t g0 = std::min<int64_t>((int64_t)b * chunk, ngroups);
    const int64_t g1 = std::min<int64_t>(g0 + chunk, ngroups);
    if (((uintptr_t)map & 15) == 0) {
      const uint4* m4 = reinterpret_cast<const uint4*>(map);
      for (int64_t g = g0 + tid; g < g1; g += kEvalThreads) {
        const uint4 q0 = m4[3 * g], q1 = m4[3 * g + 1], q2 = m4[3 * g + 2];
        const unsigned wd[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w,
                                 q2.x, q2.y, q2.z, q2.w};
        const int64_t p0 = 8 * g;
        int y = (int)(p0 / gw), x = (int)(p0 - (int64_t)y * gw);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          // samples 3j, 3j+1, 3j+2 of the 24 little-endian uint16 in wd
          const unsigned R = (wd[(3 * j) >> 1] >> (16 * ((3 * j) & 1))) & 0xffffu;
          const unsigned G = (wd[(3 * j + 1) >> 1] >> (16 * ((3 * j + 1) & 1))) & 0xffffu;
          const unsigned B = (wd[(3 * j + 2) >> 1] >> (16 * ((3 * j + 2) & 1))) & 0xffffu;
          eval_pixel(s, x, y, R, G, B, a);
          if (++x == gw) { x = 0; ++y; }
        }
      }
    } else {
      for (int64_t p = 8 * g0 + tid; p < 8 * g1; p += kEvalThreads) {
        const int y = (int)(p / gw), x = (int)(p - (int64_t)y * gw);
        eval_pixel(s, x, y, ld16(map, 3 * p), ld16(map, 3 * p + 1), ld16(map, 3 * p + 2), a);
      }
    }
    const int64_t pt = 8 * ngroups + tid;             // the scalar tail, tid < npix % 8
    if (b == P - 1 && pt < npix) {
      const int y = (int)(pt / gw), x = (int)(pt - (int64_t)y * gw);
      eval_pixel(s, x, y, ld16(map, 3 * pt), ld16(map, 3 * pt + 1), ld16(map, 3 * pt + 2), a);
    }
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    a.sum += __shfl_down(a.sum, off, kWave);
    a.valid += __shfl_down(a.valid, off, kWave);
    a.outlier += __shfl_down(a.outlier, off, kWave);
  }
  if ((tid & (kWave - 1)) == 0) {
    wsum[tid / kWave] = a.sum;
    wval[tid / kWave] = a.valid;
    wout[tid / kWave] = a.outlier;
  }
  __syncthreads();
  if (tid == 0) {
    EvalRec r = {wsum[0], wval[0], wout[0]};
#pragma unroll
    for (int k = 1; k < kEvalWaves; ++k) {
      r.sum_epe += wsum[k];
      r.n_valid += wval[k];
      r.n_outlier += wout[k];
    }
    partials[(int64_t)img * P + b] = r;
  }
}

// One wave per image: the lanes stage the image's P records into LDS, lane 0 sums them in
// index order (double) and stores the image's result.
__global__ __launch_bounds__(kWave) void flow_eval_final_kernel(
    const EvalRec* __restrict__ partials, int P, EvalRec* __restrict__ out) {
  __shared__ EvalRec part[kEvalMaxWgs];
  const int img = blockIdx.x;
  for (int i = threadIdx.x; i < P; i += kWave) part[i] = partials[(int64_t)img * P + i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  EvalRec r = {0.0, 0, 0};
  for (int i = 0; i < P; ++i) {
    r.sum_epe += part[i].sum_epe;
    r.n_valid += part[i].n_valid;
    r.n_outlier += part[i].n_outlier;
  }
  out[img] = r;
}

__global__ __launch_bounds__(256) void flow_upsample_kernel(const float* __restrict__ flow,
                                                            int n, int fh, int fw, int gh,
                                                            int gw, float2* __restrict__ out) {
  const int64_t per = (int64_t)gh * gw, total = per * n;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < total; p += stride) {
    const int img = (int)(p / per);
    const int64_t q = p - img * per;
    const int y = (int)(q / gw), x = (int)(q - (int64_t)y * gw);
    const Sampler s(flow + (int64_t)img * fh * fw * 2, fh, fw, gh, gw);
    out[p] = sample_uv(s, x, y);
  }
}

}  // namespace

extern "C" {

int of_flow_eval_partials(int n, int max_gh, int max_gw) {
  if (n <= 0) return 0;
  return (int)std::min<int64_t>((int64_t)n * partials_per_image(max_gh, max_gw), INT32_MAX);
}

int of_flow_eval(const float* flow, int n, int fh, int fw, const void* dev_gt_raw,
                 const of_image_desc* host_descs, int64_t gt_bytes, double* partials,
                 int npartials, void* out, void* stream) {
  OF_CHECK_ARG(flow && dev_gt_raw && partials && out, "flow eval: null pointer");
  OF_CHECK_ARG(n >= 0 && n <= 65535, "flow eval: n outside 0..65535");
  OF_CHECK_ARG(fh >= 1 && fw >= 1, "flow eval: flow grid size < 1");
  OF_CHECK_ARG((((uintptr_t)flow | (uintptr_t)partials | (uintptr_t)out) & 7) == 0,
               "flow eval: flow, partials and out must be 8-byte aligned");
  OF_CHECK_ARG(((uintptr_t)dev_gt_raw & 15) == 0, "flow eval: dev_gt_raw must be 16-byte aligned");
  if (n == 0) {
    OF_CHECK_ARG(npartials == 0, "flow eval: npartials is not of_flow_eval_partials(...)");
    return OF_OK;
  }
  OF_CHECK_ARG(npartials >= n && npartials % n == 0 && npartials / n <= kEvalMaxWgs,
               "flow eval: npartials is not of_flow_eval_partials(...)");
  if (host_descs)
    if (const int st = check_gt_descs("flow eval", host_descs, n, gt_bytes)) return st;
  const int P = npartials / n;
  hipLaunchKernelGGL(flow_eval_kernel, dim3(P, n), dim3(kEvalThreads), 0, as_stream(stream),
                     flow, fh, fw, static_cast<const uint8_t*>(dev_gt_raw),
                     reinterpret_cast<EvalRec*>(partials));
  if (const int st = check_launch("flow eval")) return st;
  hipLaunchKernelGGL(flow_eval_final_kernel, dim3(n), dim3(kWave), 0, as_stream(stream),
                     reinterpret_cast<const EvalRec*>(partials), P,
                     reinterpret_cast<EvalRec*>(out));
  return check_launch("flow eval (final sum)");
}

int of_flow_upsample(const float* flow, int n, int fh, int fw, int gh, int gw, float* out,
                     void* stream) {
  OF_CHECK_ARG(flow && out, "flow upsample: null pointer");
  OF_CHECK_ARG(n >= 0, "flow upsample: n < 0");
  OF_CHECK_ARG(fh >= 1 && fw >= 1 && gh >= 1 && gw >= 1, "flow upsample: size < 1");
  OF_CHECK_ARG((((uintptr_t)flow | (uintptr_t)out) & 7) == 0,
               "flow upsample: flow and out must be 8-byte aligned");
  if (n == 0) return OF_OK;
  const int64_t total = (int64_t)n * gh * gw;
  hipLaunchKernelGGL(flow_upsample_kernel, dim3((unsigned)std::min<int64_t>(cdiv(total, 256), 65536)),
                     dim3(256), 0, as_stream(stream), flow, n, fh, fw, gh, gw,
                     reinterpret_cast<float2*>(out));
  return check_launch("flow upsample");
}

}  // extern "C"
