// The bilinear sampling position of the reference's warp, shared by the feature warp and the
// loss kernels (flow_ops.hip, census_loss.hip) so that they all sample one convention.
#pragma once
#include "common.h"

namespace oflow {

// transformations.py:85-129 with the grid of model.py:65-71 (P1, P2):
//   x = i + flow0 (i = ROW index), y = j + flow1 (j = COLUMN index), sampled as column x,
//   row y; x0/x1/y0/y1 clipped; weights from the clipped x1/y1 and unclipped x/y.
// CV (OF_WARP_REFERENCE 0, OF_WARP_IMAGE 1) names the grid the flow is added to: the image
// convention adds the COLUMN index to flow0 and the ROW index to flow1 (x = j + flow0,
// y = i + flow1), everything after that being the same arithmetic.  A template parameter, so
// that the reference instantiation is the code it was.
constexpr int WARP_CV_REFERENCE = 0, WARP_CV_IMAGE = 1;
struct WarpTap {
  int64_t o00, o01, o10, o11;   // pixel offsets of (x0,y0),(x0,y1),(x1,y0),(x1,y1)
  float a, b;                   // a = x1c - x, b = y1c - y
  bool xsame, ysame;
};

template <int CV = WARP_CV_REFERENCE>
__device__ __forceinline__ WarpTap warp_tap(int i, int j, float f0, float f1, int h, int w,
                                            int64_t img, bool absolute = false) {
  WarpTap t;
  const float x = absolute ? f0 : (float)(CV == WARP_CV_IMAGE ? j : i) + f0;
  const float y = absolute ? f1 : (float)(CV == WARP_CV_IMAGE ? i : j) + f1;
  const float xf = floorf(x), yf = floorf(y);
  // float->int like tf.cast (truncation of an already-floored value), then clip.
  const int xi = (int)fmaxf(fminf(xf, 2147483520.f), -2147483520.f);
  const int yi = (int)fmaxf(fminf(yf, 2147483520.f), -2147483520.f);
  const int x0 = min(max(xi, 0), w - 1), x1 = min(max(xi + 1, 0), w - 1);
  const int y0 = min(max(yi, 0), h - 1), y1 = min(max(yi + 1, 0), h - 1);
  t.a = (float)x1 - x;
  t.b = (float)y1 - y;
  t.o00 = img + (int64_t)y0 * w + x0;
  t.o01 = img + (int64_t)y1 * w + x0;
  t.o10 = img + (int64_t)y0 * w + x1;
  t.o11 = img + (int64_t)y1 * w + x1;
  t.xsame = x0 == x1;
  t.ysame = y0 == y1;
  return t;
}

}  // namespace oflow
