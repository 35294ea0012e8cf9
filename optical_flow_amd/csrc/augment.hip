// Seeded training augmentation of the KITTI batch: of_augment_pairs takes the place of
// of_preprocess_pairs (image_ops.hip) on the reader's copy stream.  One pass over the raw
// 8-bit frames already in HBM: an affine map from the output pixel centre to a normalised
// source position (random zoom / crop, horizontal flip, rotation), a float bilinear tap with
// border replication, an optional colour stage (per-channel gain, brightness, contrast,
// saturation, clamp to [0, 1]), then the mean subtraction and pair packing of
// preprocess_pairs_kernel.  The parameters are drawn on the host (data_reader.sample_augment),
// one of_augment record per pair, shared by both images of the pair.
//
// The arithmetic is defined step by step in include/oflow.h (of_augment_pairs) and restated in
// numpy float32 by tests/augment_np.py, which the kernel matches bit for bit: IEEE single ops
// in exactly that order, floating-point contraction off, correctly rounded divisions.
#include "augment_colour.h"
#include "common.h"

#pragma clang fp contract(off)

namespace oflow {

static_assert(sizeof(of_augment) == 64, "of_augment is a 64-byte record");

// One image's three channels at output pixel centre (xc, yc).  d, a and the derived scalars are
// uniform over the workgroup (blockIdx.y picks the pair), so they live in SGPRs.
__device__ __forceinline__ void augment_pixel(const uint8_t* __restrict__ raw,
                                              const of_image_desc d, const of_augment& a, float u,
                                              float v, float val[3]) {
  const int sh = d.h, sw = d.w;
  // fmaxf / fminf drop a NaN operand, so any record (finite or not) yields in-range taps
  float sx = u * (float)sw - 0.5f;
  float sy = v * (float)sh - 0.5f;
  sx = fminf(fmaxf(sx, 0.f), (float)(sw - 1));
  sy = fminf(fmaxf(sy, 0.f), (float)(sh - 1));
  // min(): (float)(sw - 1) rounds up past 2^24
  const int x0 = min((int)floorf(sx), sw - 1), y0 = min((int)floorf(sy), sh - 1);
  const int x1 = min(x0 + 1, sw - 1), y1 = min(y0 + 1, sh - 1);
  const float fx = sx - (float)x0, fy = sy - (float)y0;
  const uint8_t* img = raw + d.offset;
  const uint8_t* r0 = img + (size_t)y0 * sw * 3;
  const uint8_t* r1 = img + (size_t)y1 * sw * 3;
  for (int c = 0; c < 3; ++c) {
    const float p00 = (float)r0[x0 * 3 + c], p01 = (float)r0[x1 * 3 + c];
    const float p10 = (float)r1[x0 * 3 + c], p11 = (float)r1[x1 * 3 + c];
    const float top = p00 + (p01 - p00) * fx;
    const float bot = p10 + (p11 - p10) * fx;
    val[c] = __fdiv_rn(top + (bot - top) * fy, 255.0f);
  }
  if (a.flags & 1) augment_colour(a, val);     // augment_colour.h, shared with selfsup.hip
}

// grid = (cdiv(oh * ow, 256), npairs): the pair's record and its two image descriptors are
// wave-uniform scalar loads; each thread writes its pixel's 24 bytes as three float2, the form
// of preprocess_pairs_kernel.  Staging the workgroup's 6 KB through LDS for lane-contiguous
// 16-byte stores measured the same within 2 % either way (data path), so the
// simpler form stays.
__global__ void __launch_bounds__(256) augment_pairs_kernel(const uint8_t* __restrict__ raw,
                                                            int oh, int ow,
                                                            const of_augment* __restrict__ params,
                                                            float* __restrict__ out) {
  const int npix = oh * ow;
  const int b = blockIdx.y;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= npix) return;
  const of_augment& a = params[b];
  const of_image_desc* descs = reinterpret_cast<const of_image_desc*>(raw);
  const float xc = (float)(pix % ow) + 0.5f, yc = (float)(pix / ow) + 0.5f;
  const float u = (a.m[0] * xc + a.m[1] * yc) + a.m[2];
  const float v = (a.m[3] * xc + a.m[4] * yc) + a.m[5];
  float o6[6];
  for (int k = 0; k < 2; ++k) {
    const of_image_desc d = descs[2 * b + k];
    float val[3] = {0.f, 0.f, 0.f};   // an absent frame: the normalised zero pixel
    if (d.h > 0 && d.w > 0) augment_pixel(raw, d, a, u, v, val);
    for (int c = 0; c < 3; ++c) o6[3 * k + c] = sub_mean(val[c], c);
  }
  float2* o = reinterpret_cast<float2*>(out + ((int64_t)b * npix + pix) * 6);
  o[0] = make_float2(o6[0], o6[1]);
  o[1] = make_float2(o6[2], o6[3]);
  o[2] = make_float2(o6[4], o6[5]);
}

int launch_augment_pairs(const void* dev_raw, int npairs, int out_h, int out_w,
                         const of_augment* dev_params, float* out, hipStream_t s) {
  if (npairs == 0) return OF_OK;
  if ((int64_t)out_h * out_w > 0x7fffffff - 256 || npairs > 65535)
    return fail(OF_EINVAL, "augment_pairs: batch too large");
  const dim3 grid((unsigned)cdiv((int64_t)out_h * out_w, 256), (unsigned)npairs);
  hipLaunchKernelGGL(augment_pairs_kernel, grid, dim3(256), 0, s,
                     static_cast<const uint8_t*>(dev_raw), out_h, out_w, dev_params, out);
  return check_launch("augment_pairs");
}

}  // namespace oflow

using namespace oflow;

extern "C" {

int of_augment_pairs(const void* dev_raw, int npairs, int out_h, int out_w,
                     const of_augment* dev_params, float* out, void* stream) {
  OF_CHECK_ARG(dev_raw && dev_params && out && npairs >= 0 && out_h > 0 && out_w > 0,
               "augment_pairs: bad arguments");
  return launch_augment_pairs(dev_raw, npairs, out_h, out_w, dev_params, out, as_stream(stream));
}

}  // extern "C"
