// The colour stage and the mean subtraction of the training augmentation, shared by
// of_augment_pairs (augment.hip: raw 8-bit frames) and of_augment_batch (selfsup.hip: a batch
// that is already preprocessed floats).  include/oflow.h (of_augment_pairs) states the
// arithmetic; both kernels are checked bit for bit against numpy float32 restatements, so every
// operation below is an IEEE single operation in the stated order, contraction off.
#pragma once
#include "common.h"

namespace oflow {

// The float64 channel means of image_ops.hip's normalise(), B G R.
__device__ __forceinline__ double channel_mean(int c) {
  return c == 0 ? 123.0 / 255.0 : c == 1 ? 117.0 / 255.0 : 104.0 / 255.0;
}

// image_ops.hip's normalise() on a float value: minus the float64 mean, rounded to float.
__device__ __forceinline__ float sub_mean(float v, int c) {
  return (float)((double)v - channel_mean(c));
}

// Its inverse on a preprocessed value: plus the float64 mean, rounded to float.
__device__ __forceinline__ float add_mean(float v, int c) {
  return (float)((double)v + channel_mean(c));
}

// Per-channel gain, brightness, contrast about 0.5, saturation about the pixel's gray, clamp to
// [0, 1], on the three channels of one pixel in [0, 1].
__device__ __forceinline__ void augment_colour(const of_augment& a, float val[3]) {
#pragma clang fp contract(off)
  for (int c = 0; c < 3; ++c) {
    val[c] *= a.gain[c];
    val[c] += a.brightness;
    val[c] = (val[c] - 0.5f) * a.contrast + 0.5f;
  }
  const float gray = (0.114f * val[0] + 0.587f * val[1]) + 0.299f * val[2];
  for (int c = 0; c < 3; ++c) {
    val[c] = gray + (val[c] - gray) * a.saturation;
    val[c] = fminf(fmaxf(val[c], 0.f), 1.f);
  }
}

}  // namespace oflow
