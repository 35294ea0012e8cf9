// Augmentation self-supervision (build-added; ARFlow's "augmentation as regularisation", UFlow's
// "teacher sees the full frame, student sees a crop"): the net's own flow on the un-augmented
// batch is carried through a random crop / zoom / flip / rotation and becomes the target of the
// flow the net predicts on the transformed batch.  Three pixelwise kernels, image convention
// only; include/oflow.h states their arithmetic:
//   of_augment_batch         the of_augment map and colour stage of of_augment_pairs on a batch
//                            that is already preprocessed floats (bit-exact against
//                            tests/selfsup_ref.py: IEEE single ops in the stated order,
//                            contraction off);
//   of_flow_transform        the teacher flow sampled where each student cell lies on the
//                            teacher grid, mapped through the inverse linear part of the record,
//                            and the weight inside * visible * teacher mask;
//   of_flow_distill_fwd      the weighted generalised Charbonnier flow-to-flow penalty, its
//                            per-workgroup partials and its gradient plane in one pass.
// No atomics, no allocation, no host read; every output element is written.
#include <cmath>

#include "augment_colour.h"
#include "common.h"

namespace oflow {

static_assert(sizeof(of_augment) == 64, "of_augment is a 64-byte record");

// The clamped bilinear taps of one axis: s clamped to [0, size-1] (fmaxf / fminf drop a NaN
// operand, so any record yields in-range taps), i0 = floor, i1 = min(i0+1, size-1), f = s - i0.
__device__ __forceinline__ void axis_taps(float s, int size, int& i0, int& i1, float& f) {
  s = fminf(fmaxf(s, 0.f), (float)(size - 1));
  i0 = min((int)floorf(s), size - 1);     // min(): (float)(size - 1) rounds up past 2^24
  i1 = min(i0 + 1, size - 1);
  f = s - (float)i0;
}

// grid = (cdiv(h * w, 256), n): image b's record is a wave-uniform scalar load; a thread reads
// its pixel's four taps (24 bytes each, three float2) and writes 24 bytes as three float2, the
// form of augment_pairs_kernel.
__global__ void __launch_bounds__(256) augment_batch_kernel(const float* __restrict__ batch, int h,
                                                            int w,
                                                            const of_augment* __restrict__ params,
                                                            float* __restrict__ out) {
#pragma clang fp contract(off)
  const int npix = h * w;
  const int b = blockIdx.y;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= npix) return;
  const of_augment& a = params[b];
  const float xc = (float)(pix % w) + 0.5f, yc = (float)(pix / w) + 0.5f;
  const float u = (a.m[0] * xc + a.m[1] * yc) + a.m[2];
  const float v = (a.m[3] * xc + a.m[4] * yc) + a.m[5];
  int x0, x1, y0, y1;
  float fx, fy;
  axis_taps(u * (float)w - 0.5f, w, x0, x1, fx);
  axis_taps(v * (float)h - 0.5f, h, y0, y1, fy);
  const float2* img = reinterpret_cast<const float2*>(batch) + (int64_t)b * npix * 3;
  const float2* t00 = img + ((int64_t)y0 * w + x0) * 3;
  const float2* t01 = img + ((int64_t)y0 * w + x1) * 3;
  const float2* t10 = img + ((int64_t)y1 * w + x0) * 3;
  const float2* t11 = img + ((int64_t)y1 * w + x1) * 3;
  float o6[6];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float2 p00 = t00[k], p01 = t01[k], p10 = t10[k], p11 = t11[k];
    const float topx = p00.x + (p01.x - p00.x) * fx, botx = p10.x + (p11.x - p10.x) * fx;
    const float topy = p00.y + (p01.y - p00.y) * fx, boty = p10.y + (p11.y - p10.y) * fx;
    o6[2 * k] = topx + (botx - topx) * fy;
    o6[2 * k + 1] = topy + (boty - topy) * fy;
  }
  if (a.flags & 1) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      float val[3];
      for (int c = 0; c < 3; ++c) val[c] = add_mean(o6[3 * k + c], c);
      augment_colour(a, val);
      for (int c = 0; c < 3; ++c) o6[3 * k + c] = sub_mean(val[c], c);
    }
  }
  float2* o = reinterpret_cast<float2*>(out) + ((int64_t)b * npix + pix) * 3;
  o[0] = make_float2(o6[0], o6[1]);
  o[1] = make_float2(o6[2], o6[3]);
  o[2] = make_float2(o6[4], o6[5]);
}

// grid = (cdiv(fh * fw, 256), n): one thread per student cell; the record, the cell -> image
// scale and the inverse of the map's linear part are wave-uniform.
__global__ void __launch_bounds__(256) flow_transform_kernel(
    const float2* __restrict__ teacher, int fh, int fw, int img_h, int img_w,
    const of_augment* __restrict__ params, const float* __restrict__ mask,
    float2* __restrict__ target, float* __restrict__ weight) {
  const int ncell = fh * fw;
  const int b = blockIdx.y;
  const int cell = blockIdx.x * 256 + threadIdx.x;
  if (cell >= ncell) return;
  const of_augment& r = params[b];
  const int i = cell / fw, j = cell - i * fw;
  const float xc = ((float)j + 0.5f) * (float)img_w / (float)fw;
  const float yc = ((float)i + 0.5f) * (float)img_h / (float)fh;
  const float u = (r.m[0] * xc + r.m[1] * yc) + r.m[2];
  const float v = (r.m[3] * xc + r.m[4] * yc) + r.m[5];
  const float px = u * (float)fw - 0.5f, py = v * (float)fh - 0.5f;
  int x0, x1, y0, y1;
  float fx, fy;
  axis_taps(px, fw, x0, x1, fx);
  axis_taps(py, fh, y0, y1, fy);
  const int64_t base = (int64_t)b * ncell;
  const int64_t o00 = base + (int64_t)y0 * fw + x0, o01 = base + (int64_t)y0 * fw + x1;
  const int64_t o10 = base + (int64_t)y1 * fw + x0, o11 = base + (int64_t)y1 * fw + x1;
  const float2 p00 = teacher[o00], p01 = teacher[o01], p10 = teacher[o10], p11 = teacher[o11];
  const float topx = p00.x + (p01.x - p00.x) * fx, botx = p10.x + (p11.x - p10.x) * fx;
  const float topy = p00.y + (p01.y - p00.y) * fx, boty = p10.y + (p11.y - p10.y) * fx;
  const float tx = topx + (botx - topx) * fy, ty = topy + (boty - topy) * fy;
  const float xmax = (float)(fw - 1), ymax = (float)(fh - 1);
  const bool inside = px >= 0.f && px <= xmax && py >= 0.f && py <= ymax;
  const float qx = px + tx, qy = py + ty;
  const bool visible = qx >= 0.f && qx <= xmax && qy >= 0.f && qy <= ymax;
  // A: the map's linear part in cells (student cell step -> teacher cell step)
  const float a00 = r.m[0] * (float)img_w, a01 = r.m[1] * (float)img_h * (float)fw / (float)fh;
  const float a10 = r.m[3] * (float)img_w * (float)fh / (float)fw, a11 = r.m[4] * (float)img_h;
  const float det = a00 * a11 - a01 * a10;
  float2 tg = make_float2(0.f, 0.f);
  float wt = 0.f;
  if (fabsf(det) >= 1e-12f) {              // (false for a NaN determinant too)
    tg.x = (a11 * tx - a01 * ty) / det;
    tg.y = (a00 * ty - a10 * tx) / det;
    if (inside && visible) {
      wt = 1.f;
      if (mask) {
        const float m00 = mask[o00], m01 = mask[o01], m10 = mask[o10], m11 = mask[o11];
        const float top = m00 + (m01 - m00) * fx, bot = m10 + (m11 - m10) * fx;
        wt = top + (bot - top) * fy;
      }
    }
  }
  target[base + cell] = tg;
  weight[base + cell] = wt;
}

constexpr int kDistThreads = 256;
constexpr int kDistCells = 1024;          // cells per workgroup: two rounds of two per thread

// w * (|s - t|^2 + eps^2)^(q/2) of one cell and its gradient g = coef * d / d s; a cell of
// weight 0 contributes exactly 0 to both.
__device__ __forceinline__ float distill_cell(float sx, float sy, float tx, float ty, float w,
                                              float hq, float q, float eps2, float coef,
                                              float& gx, float& gy) {
  gx = gy = 0.f;
  if (w == 0.f) return 0.f;
  const float ex = sx - tx, ey = sy - ty;
  const float r2 = ex * ex + ey * ey + eps2;
  // r2^(q/2) as exp2f(q/2 log2f(r2)), the supervised term's form
  const float rho = q == 1.f ? sqrtf(r2) : exp2f(hq * log2f(r2));
  const float g = coef * w * (q * rho / r2);
  gx = g * ex;
  gy = g * ey;
  return w * rho;
}

// One workgroup = kDistCells consecutive cells.  VEC: a thread takes two neighbouring cells per
// round with 16-byte flow loads / stores and an 8-byte weight load (lane-contiguous); else one
// float2 per cell (pointers that are only 8 / 4-byte aligned).  Sums: per thread in double, a
// wave shuffle tree, the four waves through LDS in wave order, one partial per workgroup.
template <bool VEC>
__global__ void __launch_bounds__(kDistThreads) flow_distill_kernel(
    const float* __restrict__ student, const float* __restrict__ target,
    const float* __restrict__ weight, int total, float hq, float q, float eps2, float coef,
    float* __restrict__ plane, float* __restrict__ partials) {
  __shared__ double s_red[kDistThreads / kWave];
  const int tid = threadIdx.x;
  double acc = 0.0;
#pragma unroll
  for (int round = 0; round < kDistCells / (2 * kDistThreads); ++round) {
    const int cell = blockIdx.x * kDistCells + 2 * (round * kDistThreads + tid);
    if (VEC && cell + 1 < total) {
      const float4 s = *reinterpret_cast<const float4*>(student + 2 * (int64_t)cell);
      const float4 t = *reinterpret_cast<const float4*>(target + 2 * (int64_t)cell);
      const float2 w = *reinterpret_cast<const float2*>(weight + cell);
      float4 g;
      acc += (double)distill_cell(s.x, s.y, t.x, t.y, w.x, hq, q, eps2, coef, g.x, g.y);
      acc += (double)distill_cell(s.z, s.w, t.z, t.w, w.y, hq, q, eps2, coef, g.z, g.w);
      if (plane) *reinterpret_cast<float4*>(plane + 2 * (int64_t)cell) = g;
    } else {
      for (int k = 0; k < 2; ++k) {
        const int c = cell + k;
        if (c >= total) break;
        const float2 s = *reinterpret_cast<const float2*>(student + 2 * (int64_t)c);
        const float2 t = *reinterpret_cast<const float2*>(target + 2 * (int64_t)c);
        float2 g;
        acc += (double)distill_cell(s.x, s.y, t.x, t.y, weight[c], hq, q, eps2, coef, g.x, g.y);
        if (plane) *reinterpret_cast<float2*>(plane + 2 * (int64_t)c) = g;
      }
    }
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, kWave);
  if ((tid & (kWave - 1)) == 0) s_red[tid / kWave] = acc;
  __syncthreads();
  if (tid == 0) {
    double tot = s_red[0];
#pragma unroll
    for (int k = 1; k < kDistThreads / kWave; ++k) tot += s_red[k];
    partials[blockIdx.x] = (float)((double)coef * tot);
  }
}

}  // namespace oflow

using namespace oflow;

extern "C" {

int of_augment_batch(const float* batch, int n, int h, int w, const of_augment* dev_params,
                     float* out, void* stream) {
  OF_CHECK_ARG(batch && dev_params && out && n >= 0 && h > 0 && w > 0,
               "augment_batch: bad arguments");
  OF_CHECK_ARG(batch != out, "augment_batch: cannot run in place");
  OF_CHECK_ARG(!((uintptr_t)batch & 7) && !((uintptr_t)out & 7) && !((uintptr_t)dev_params & 3),
               "augment_batch: batch and out must be 8-byte aligned");
  if (n == 0) return OF_OK;
  if ((int64_t)h * w > 0x7fffffff - 256 || n > 65535)
    return fail(OF_EINVAL, "augment_batch: batch too large");
  const dim3 grid((unsigned)cdiv((int64_t)h * w, 256), (unsigned)n);
  hipLaunchKernelGGL(augment_batch_kernel, grid, dim3(256), 0, as_stream(stream), batch, h, w,
                     dev_params, out);
  return check_launch("augment_batch");
}

int of_flow_transform(const float* teacher, int n, int fh, int fw, int img_h, int img_w,
                      const of_augment* dev_params, const float* teacher_mask, float* target,
                      float* weight, void* stream) {
  OF_CHECK_ARG(teacher && dev_params && target && weight, "flow_transform: NULL argument");
  OF_CHECK_ARG(n >= 0 && fh > 0 && fw > 0 && img_h > 0 && img_w > 0,
               "flow_transform: n < 0 or a size < 1");
  OF_CHECK_ARG(!((uintptr_t)teacher & 7) && !((uintptr_t)target & 7) &&
                   !((uintptr_t)weight & 3) && !((uintptr_t)teacher_mask & 3) &&
                   !((uintptr_t)dev_params & 3),
               "flow_transform: teacher and target must be 8-byte aligned");
  OF_CHECK_ARG(teacher != target, "flow_transform: cannot run in place");
  if (n == 0) return OF_OK;
  if ((int64_t)fh * fw > 0x7fffffff - 256 || n > 65535)
    return fail(OF_EINVAL, "flow_transform: batch too large");
  const dim3 grid((unsigned)cdiv((int64_t)fh * fw, 256), (unsigned)n);
  hipLaunchKernelGGL(flow_transform_kernel, grid, dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const float2*>(teacher), fh, fw, img_h, img_w, dev_params,
                     teacher_mask, reinterpret_cast<float2*>(target), weight);
  return check_launch("flow_transform");
}

int of_flow_distill_partials(int n, int fh, int fw) {
  if (n < 1 || fh < 1 || fw < 1) return 0;
  const int64_t total = (int64_t)n * fh * fw;
  if (total > 0x7fffffff - kDistCells) return 0;
  return (int)cdiv(total, kDistCells);
}

int of_flow_distill_fwd(const float* student, const float* target, const float* weight, int n,
                        int fh, int fw, float q, float eps, float coef, float* plane,
                        float* partials, void* stream) {
  static const std::string fn = "of_flow_distill_fwd";
  if (!student || !target || !weight || !partials) return fail(OF_EINVAL, fn + ": NULL argument");
  if (n < 1 || fh < 1 || fw < 1) return fail(OF_EINVAL, fn + ": n or a grid size < 1");
  if ((int64_t)n * fh * fw > 0x7fffffff - kDistCells)
    return fail(OF_EINVAL, fn + ": n * fh * fw must stay under 2^31 - 1024");
  if (!(q > 0.f && q <= 2.f)) return fail(OF_EINVAL, fn + ": q must be in (0, 2]");
  if (!(eps > 0.f) || !std::isfinite(eps)) return fail(OF_EINVAL, fn + ": eps must be > 0");
  if (((uintptr_t)student & 7) || ((uintptr_t)target & 7) || ((uintptr_t)plane & 7) ||
      ((uintptr_t)weight & 3) || ((uintptr_t)partials & 3))
    return fail(OF_EINVAL, fn + ": flows and plane must be 8-byte, weight and partials 4-byte "
                                "aligned");
  const int total = n * fh * fw;
  const bool vec = !((uintptr_t)student & 15) && !((uintptr_t)target & 15) &&
                   !((uintptr_t)plane & 15) && !((uintptr_t)weight & 7);
  const dim3 grid((unsigned)cdiv(total, kDistCells));
  hipLaunchKernelGGL(vec ? flow_distill_kernel<true> : flow_distill_kernel<false>, grid,
                     dim3(kDistThreads), 0, as_stream(stream), student, target, weight, total,
                     0.5f * q, q, eps * eps, coef, plane, partials);
  return check_launch("flow_distill_fwd");
}

}  // extern "C"
