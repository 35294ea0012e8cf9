// Global-norm gradient clipping and the non-finite update guard for Keras Adam
// (tf.keras.optimizers.Adam(global_clipnorm=...), i.e. tf.clip_by_global_norm over every
// gradient): a deterministic sum of squares of the gradient arena, and a sibling of
// adam_sched_kernel + adam_dev_kernel (misc.hip) that reads the gradient multiplier and the
// skip decision from a device state block.  Nothing here returns to the host, so the update
// stays capturable (HIP graph) and every data-parallel rank decides alike from equal bytes.
#include <algorithm>
#include <cmath>

#include "common.h"

using namespace oflow;

namespace {

constexpr int kSumsqThreads = 1024;               // 16 waves: one workgroup fills a CU's loads
constexpr int kSumsqWaves = kSumsqThreads / kWave;
constexpr int64_t kSumsqPerWg = 16384;            // floats per workgroup before P saturates
constexpr int kSumsqMinWgs = 64, kSumsqMaxWgs = 256;

// P(n): 64 up to 1 Mi floats, then one workgroup per 16 Ki floats, at most 256 (one per CU of
// a whole MI355X; the full 4.94 M arena runs 256).  A function of n alone.
int sumsq_partials(int64_t n) {
  return (int)std::min<int64_t>(std::max<int64_t>(cdiv(n, kSumsqPerWg), kSumsqMinWgs),
                                kSumsqMaxWgs);
}

// The device state block (of_adam_clip_state_bytes): written by adam_clip_sched_kernel, read
// by adam_clip_kernel and, through views, by the host.
struct ClipState {
  double norm;            // grad_scale * sqrt(sum of squares)
  float norm_f;           // (float)norm
  float mult;             // the effective gradient multiplier of this step
  int32_t skip;           // 1: this step's update was skipped (non-finite norm, guard on)
  int32_t skipped_total;  // running count of skipped updates
  int32_t pad[2];
};
static_assert(sizeof(ClipState) == 32, "ClipState layout is part of the ABI");

// Workgroup b owns the float4 quads [b*chunk, min((b+1)*chunk, n/4)), chunk = ceil(n/4 / P);
// the last workgroup also owns the n % 4 scalars after the last quad.  g^2 is formed and summed
// in double (a float's square is exact there: no overflow at 1e25, no underflow at 1e-30).
// Fixed order: a thread sums its quads in index order (one accumulator per component, combined
// x, y, z, w), a wave reduces by a shuffle tree, thread 0 sums the 16 wave sums in wave order.
// One plain store per workgroup; an empty range stores 0.
__global__ __launch_bounds__(kSumsqThreads) void grad_sumsq_kernel(const float* __restrict__ g,
                                                                    int64_t n,
                                                                    double* __restrict__ partials) {
  __shared__ double wsum[kSumsqWaves];
  const int tid = threadIdx.x;
  const int64_t nq = n / 4;
  const int64_t chunk = (nq + gridDim.x - 1) / gridDim.x;
  const int64_t q0 = std::min<int64_t>((int64_t)blockIdx.x * chunk, nq);
  const int64_t q1 = std::min<int64_t>(q0 + chunk, nq);
  double ax = 0.0, ay = 0.0, az = 0.0, aw = 0.0;
  const float4* g4 = reinterpret_cast<const float4*>(g);
#pragma unroll 4
  for (int64_t i = q0 + tid; i < q1; i += kSumsqThreads) {
    const float4 v = g4[i];
    const double x = v.x, y = v.y, z = v.z, w = v.w;
    ax = fma(x, x, ax);
    ay = fma(y, y, ay);
    az = fma(z, z, az);
    aw = fma(w, w, aw);
  }
  double acc = ((ax + ay) + az) + aw;
  if (blockIdx.x == gridDim.x - 1 && 4 * nq + tid < n) {      // the scalar tail, tid < n % 4
    const double x = g[4 * nq + tid];
    acc = fma(x, x, acc);
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, kWave);
  if ((tid & (kWave - 1)) == 0) wsum[tid / kWave] = acc;
  __syncthreads();
  if (tid == 0) {
    double s = wsum[0];
#pragma unroll
    for (int k = 1; k < kSumsqWaves; ++k) s += wsum[k];
    partials[blockIdx.x] = s;
  }
}

// One wave.  The lanes stage the P partials into LDS; lane 0 sums them in index order, forms
// the norm, the multiplier and the skip decision, and -- unless the step is skipped -- advances
// the schedule exactly as adam_sched_kernel does.
__global__ __launch_bounds__(kWave) void adam_clip_sched_kernel(
    float* __restrict__ sched, int32_t* __restrict__ iter, float b1, float b2, float gs,
    const double* __restrict__ partials, int np, float clip_norm, int skip_nonfinite,
    ClipState* __restrict__ st) {
  __shared__ double part[kSumsqMaxWgs];
  for (int i = threadIdx.x; i < kSumsqMaxWgs; i += kWave) part[i] = i < np ? partials[i] : 0.0;
  __syncthreads();
  if (threadIdx.x != 0) return;
  // index order, 16 LDS reads in flight per round; the zero padding past np adds +0.0, which
  // changes no sum (the sum starts at +0.0, so it is never -0.0)
  double sum = 0.0;
  for (int i = 0; i < np; i += 16) {
    double t[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) t[k] = part[i + k];
#pragma unroll
    for (int k = 0; k < 16; ++k) sum += t[k];
  }
  const double norm = (double)gs * sqrt(sum);
  const bool finite = isfinite(norm);
  const int skip = (!finite && skip_nonfinite) ? 1 : 0;
  float mult = gs;
  if (clip_norm > 0.f) {
    // TF's clip_norm * min(1/norm, 1/clip_norm); gs * clip_norm is exact in double, so a norm
    // at or under clip_norm gives mult == gs bitwise.  Non-finite norm: NaN, as
    // tf.clip_by_global_norm documents (with the guard off; a skipped step keeps gs, unused).
    const double c = clip_norm;
    if (finite)
      mult = (float)((double)gs * c / fmax(norm, c));
    else if (!skip)
      mult = __builtin_nanf("");
  }
  st->norm = norm;
  st->norm_f = (float)norm;
  st->mult = mult;
  st->skip = skip;
  st->skipped_total += skip;
  if (skip) return;                     // *iter and sched[1] stay: the next step gets this t
  const int t = *iter + 1;
  *iter = t;
  const double lr = sched[0];
  sched[1] = (float)(lr * sqrt(1.0 - pow((double)b2, (double)t)) / (1.0 - pow((double)b1, (double)t)));
}

// adam_dev_kernel (misc.hip) with the gradient multiplier read from the state block, and
// nothing touched when the step is skipped.
__global__ __launch_bounds__(256) void adam_clip_kernel(float* __restrict__ p,
                                                        const float* __restrict__ g,
                                                        float* __restrict__ m,
                                                        float* __restrict__ v, int64_t n,
                                                        const float* __restrict__ sched, float b1,
                                                        float b2, float eps,
                                                        const ClipState* __restrict__ st) {
  if (st->skip) return;
  const float gs = st->mult;
  const float lr_t = sched[1];
  const int64_t nq = n / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t i = tid; i < nq; i += stride) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    float4 gg = reinterpret_cast<const float4*>(g)[i];
    gg.x *= gs; gg.y *= gs; gg.z *= gs; gg.w *= gs;
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
#define OF_ADAM1(c)                                  \
  mm.c += (gg.c - mm.c) * (1.f - b1);                \
  vv.c += (gg.c * gg.c - vv.c) * (1.f - b2);         \
  pp.c -= lr_t * mm.c / (sqrtf(vv.c) + eps);
    OF_ADAM1(x) OF_ADAM1(y) OF_ADAM1(z) OF_ADAM1(w)
#undef OF_ADAM1
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
  for (int64_t i = 4 * nq + tid; i < n; i += stride) {
    const float gi = g[i] * gs;
    m[i] += (gi - m[i]) * (1.f - b1);
    v[i] += (gi * gi - v[i]) * (1.f - b2);
    p[i] -= lr_t * m[i] / (sqrtf(v[i]) + eps);
  }
}

}  // namespace

extern "C" {

int of_grad_sumsq_partials(int64_t n) { return sumsq_partials(n < 0 ? 0 : n); }

size_t of_adam_clip_state_bytes(void) { return sizeof(ClipState); }

int of_grad_sumsq(const float* g, int64_t n, double* partials, void* stream) {
  OF_CHECK_ARG(g && partials, "grad sumsq: null pointer");
  OF_CHECK_ARG(n >= 0, "grad sumsq: n < 0");
  OF_CHECK_ARG(((uintptr_t)g & 15) == 0, "grad sumsq: g must be 16-byte aligned");
  OF_CHECK_ARG(((uintptr_t)partials & 7) == 0, "grad sumsq: partials must be 8-byte aligned");
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(sumsq_partials(n)), dim3(kSumsqThreads), 0,
                     as_stream(stream), g, n, partials);
  return check_launch("grad sumsq");
}

int of_adam_keras_dev_clip(float* p, const float* g, float* m, float* v, int64_t n, float* sched,
                           int32_t* iter, float beta1, float beta2, float eps, float grad_scale,
                           const double* partials, int npartials, float clip_norm,
                           int skip_nonfinite, void* state, void* stream) {
  OF_CHECK_ARG(p && g && m && v && sched && iter && partials && state,
               "adam clip: null pointer");
  OF_CHECK_ARG(n >= 0, "adam clip: n < 0");
  OF_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0,
               "adam clip: arenas must be 16-byte aligned");
  OF_CHECK_ARG((((uintptr_t)partials | (uintptr_t)state) & 7) == 0,
               "adam clip: partials and state must be 8-byte aligned");
  OF_CHECK_ARG(npartials == sumsq_partials(n),
               "adam clip: npartials is not of_grad_sumsq_partials(n)");
  OF_CHECK_ARG(clip_norm >= 0.f, "adam clip: clip_norm negative or NaN");   // NaN fails >=
  hipLaunchKernelGGL(adam_clip_sched_kernel, dim3(1), dim3(kWave), 0, as_stream(stream), sched,
                     iter, beta1, beta2, grad_scale, partials, npartials, clip_norm,
                     skip_nonfinite, reinterpret_cast<ClipState*>(state));
  if (n > 0)
    hipLaunchKernelGGL(adam_clip_kernel, dim3(std::min<int64_t>(cdiv(n / 4 + 1, 256), 2048)),
                       dim3(256), 0, as_stream(stream), p, g, m, v, n, sched, beta1, beta2, eps,
                       reinterpret_cast<const ClipState*>(state));
  return check_launch("adam clip");
}

}  // extern "C"
