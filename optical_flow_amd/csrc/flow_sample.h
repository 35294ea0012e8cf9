// The half-pixel bilinear sampler of a flow grid at a native-size pixel, shared by the
// evaluation (flow_eval.hip: of_flow_eval, of_flow_upsample) and the supervised term
// (supervised_loss.hip): one set of __device__ functions, so all of them compare the same
// number.  include/oflow.h (of_flow_eval) states the arithmetic.
#pragma once
#include "common.h"

namespace oflow {

// The flow grid and one image's size, with the ratios the sampler needs.
struct Sampler {
  const float* flow;      // this image's (fh, fw, 2)
  int fh, fw, gh, gw;
  float ku, kv;           // gw / fw, gh / fh: flow-grid pixels -> native pixels
  __device__ Sampler(const float* f, int fh_, int fw_, int gh_, int gw_)
      : flow(f), fh(fh_), fw(fw_), gh(gh_), gw(gw_), ku((float)gw_ / (float)fw_),
        kv((float)gh_ / (float)fh_) {}
};

// Floor i0 and fraction f of the source coordinate s = (i + 0.5) n / g - 0.5 clamped to
// [0, n-1], from the exact integers s = ((2 i + 1) n - g) / (2 g): the float quotient only
// proposes the floor, the integer remainder corrects it and gives the fraction with one
// rounding.  (Formed in fp32, s carries half an ulp of its own size, 1.5e-5 at 1242 columns,
// and a flow that changes by 80 px from one cell to the next turns that into 1.2e-3 px.)
__device__ __forceinline__ void src_coord(int i, int n, int g, int& i0, float& f) {
  const int64_t D = 2 * (int64_t)g;
  const int64_t N = (2 * (int64_t)i + 1) * n - g;
  i0 = 0;
  f = 0.f;
  if (N <= 0) return;                               // left of the first centre: replicate
  int64_t q = (int64_t)((float)N / (float)D);
  int64_t r = N - q * D;
  while (r < 0) { --q; r += D; }
  while (r >= D) { ++q; r -= D; }
  if (q >= n - 1) { i0 = n - 1; return; }           // at or past the last centre
  i0 = (int)q;
  f = (float)r / (float)D;
}

// The interpolation of the four taps and the scaling to native pixels.
__device__ __forceinline__ float2 bilerp_uv(float2 p00, float2 p01, float2 p10, float2 p11,
                                            float fx, float fy, float ku, float kv) {
  const float tx = p00.x + (p01.x - p00.x) * fx, bx = p10.x + (p11.x - p10.x) * fx;
  const float ty = p00.y + (p01.y - p00.y) * fx, by = p10.y + (p11.y - p10.y) * fx;
  return make_float2((tx + (bx - tx) * fy) * ku, (ty + (by - ty) * fy) * kv);
}

// (u, v) of ground-truth pixel (x, y), the taps read from the flow in global memory.
__device__ __forceinline__ float2 sample_uv(const Sampler& s, int x, int y) {
  int x0, y0;
  float fx, fy;
  src_coord(x, s.fw, s.gw, x0, fx);
  src_coord(y, s.fh, s.gh, y0, fy);
  const int x1 = min(x0 + 1, s.fw - 1), y1 = min(y0 + 1, s.fh - 1);
  const float2* f2 = reinterpret_cast<const float2*>(s.flow);
  const float2 p00 = f2[(int64_t)y0 * s.fw + x0], p01 = f2[(int64_t)y0 * s.fw + x1];
  const float2 p10 = f2[(int64_t)y1 * s.fw + x0], p11 = f2[(int64_t)y1 * s.fw + x1];
  return bilerp_uv(p00, p01, p10, p11, fx, fy, s.ku, s.kv);
}

// uint16 sample k of a map at any byte address.
__device__ __forceinline__ unsigned ld16(const uint8_t* p, int64_t k) {
  return (unsigned)p[2 * k] | ((unsigned)p[2 * k + 1] << 8);
}

}  // namespace oflow
