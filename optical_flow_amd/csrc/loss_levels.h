// The "up to 8 pyramid levels in one launch" table of the loss and mask kernels, and what every
// one of them does with it: find the level of a block or pixel id, decode a tile, reduce a
// block's floats in a fixed order, check the per-level arguments on the host.  The per-term
// structs derive from LevelTable and add only their pointers, coefficients and row strides.
#pragma once
#include <algorithm>
#include <string>

#include "common.h"

namespace oflow {

// Level l's ids are [beg[l], beg[l+1]): pixels, blocks of pixels, or the tiles of a tx[l] x
// ty[l] grid per image (image-major, then tile row, then tile column): levels_by_*() say which.
struct LevelTable {
  int h[8], w[8];
  int tx[8], ty[8];
  int64_t beg[9];
  int levels;
};

__device__ __forceinline__ int level_of(const LevelTable& m, int64_t id) {
  int l = 0;
  while (l + 1 < m.levels && id >= m.beg[l + 1]) ++l;
  return l;
}

// Tile ``id`` of level l, TY x TX pixels: its origin and its image's pixel offset.
template <int TY, int TX>
__device__ __forceinline__ void tile_of(const LevelTable& m, int l, int64_t id, int64_t& img,
                                        int& y0, int& x0) {
  int t = (int)(id - m.beg[l]);
  x0 = (t % m.tx[l]) * TX;
  t /= m.tx[l];
  y0 = (t % m.ty[l]) * TY;
  img = (int64_t)(t / m.ty[l]) * m.h[l] * m.w[l];
}

// The sum of ``s`` over a block of THREADS threads, in thread 0 (0 elsewhere), in a fixed
// order: xor shuffles within each wave, one LDS float per wave, added in wave order.  No
// atomics, so a kernel's partials are run-to-run bitwise equal.
template <int THREADS>
__device__ __forceinline__ float block_sum_fixed(float s) {
  __shared__ float red[THREADS / 64];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  float t = 0.f;
  if (threadIdx.x == 0)
    for (int k = 0; k < THREADS / 64; ++k) t += red[k];
  return t;
}

// levels, n, hs, ws and the size limit of a level; fills h, w and levels.  ``f``: the entry's
// name, the prefix of every message; ``size``: what the entry calls a level size below 1.
inline int levels_init(const std::string& f, int n, const int* hs, const int* ws, int levels,
                       LevelTable& m, const char* size = "h or w < 1") {
  if (levels < 1 || levels > 8) return fail(OF_EINVAL, f + ": levels must be 1..8");
  if (!hs || !ws) return fail(OF_EINVAL, f + ": NULL argument");
  if (n < 1) return fail(OF_EINVAL, f + ": n < 1");
  m.levels = levels;
  for (int l = 0; l < levels; ++l) {
    if (hs[l] < 1 || ws[l] < 1) return fail(OF_EINVAL, f + ": " + size);
    if ((int64_t)n * hs[l] * ws[l] >= (1LL << 40))
      return fail(OF_EINVAL, f + ": a level must hold < 2^40 pixels");
    m.h[l] = hs[l];
    m.w[l] = ws[l];
  }
  return OF_OK;
}

// beg[] after levels_init(), one id per ``pixels`` pixels of a level: 1 for the pixel kernels
// (a grid-stride loop walks them), a block's share for kernels that launch one workgroup per
// id, which must then fit a grid.
inline int levels_by_pixels(const std::string& f, int n, LevelTable& m, int pixels = 1) {
  m.beg[0] = 0;
  for (int l = 0; l < m.levels; ++l)
    m.beg[l + 1] = m.beg[l] + cdiv((int64_t)n * m.h[l] * m.w[l], pixels);
  if (pixels > 1 && m.beg[m.levels] >= INT32_MAX)
    return fail(OF_EINVAL, f + ": too many blocks");
  return OF_OK;
}

// beg[] and the tile table after levels_init(): one workgroup per ty x tx tile of each image.
inline int levels_by_tiles(const std::string& f, int n, LevelTable& m, int ty, int tx) {
  m.beg[0] = 0;
  for (int l = 0; l < m.levels; ++l) {
    m.tx[l] = (int)cdiv(m.w[l], tx);
    m.ty[l] = (int)cdiv(m.h[l], ty);
    m.beg[l + 1] = m.beg[l] + (int64_t)n * m.ty[l] * m.tx[l];
  }
  if (m.beg[m.levels] >= INT32_MAX) return fail(OF_EINVAL, f + ": too many blocks");
  return OF_OK;
}

// A per-level array of flow or plane pointers (float2 per pixel): none NULL, all 8-byte aligned.
inline int levels_ptrs8(const std::string& f, const float* const* ps, int levels,
                        const char* what) {
  for (int l = 0; l < levels; ++l)
    if (!ps[l] || ((uintptr_t)ps[l] & 7))
      return fail(OF_EINVAL, f + ": NULL or not 8-byte aligned " + what);
  return OF_OK;
}

// The grid of a grid-stride loop over ``work`` items.
inline int grid_for(int64_t work, int per_block = 256, int cap = 8192) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(work, per_block), cap));
}

// planes[l] (n, h, w, 2), scaled by coefs[l] * dloss[0] (dloss NULL: 1), written to or added
// into dflows[l] at row stride lds[l]: the backward of every term whose forward leaves its
// d(term)/d(flow) as a dense plane (census, SSIM, supervised, self-supervision).  Defined in
// loss_levels.hip; ``f`` is the calling entry's name.
int plane_scale_multi(const std::string& f, const float* const* planes, int n, const int* hs,
                      const int* ws, int levels, const float* coefs, const float* dloss,
                      float* const* dflows, const int* lds, int accumulate, void* stream);

}  // namespace oflow
