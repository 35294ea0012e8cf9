// Labelled augmentation (build-added; the reference trains without labels and without
// augmentation): of_gt_augment moves a raw ground-truth batch -- of_flow_eval's sparse 16-bit
// KITTI flow maps, each at its own size -- through the of_augment records that
// of_augment_pairs moves the frames through, so a crop, zoom or flip of a labelled frame keeps
// its truth.  include/oflow.h states the arithmetic; tests/gt_augment_ref.py restates it bit
// for bit in numpy float32 (IEEE single ops in the stated order, contraction off, correctly
// rounded divisions) and independently in float64.
//
// A gather, never a blend: an output pixel takes the one source pixel its centre falls into.
// A bilinear tap would mix valid and invalid neighbours and average vectors across motion
// boundaries; the vector then goes through the inverse of the map's linear part.
//
// Shape: a map is a dense run of 6-byte pixels (of_flow_eval's view).  A thread owns eight
// consecutive output pixels = 48 bytes = three 16-byte stores.  Six-byte pixels meet a
// 16-byte boundary every eight pixels, so a map at any even address has a head of at most
// seven pixels after which its groups of eight are 16-byte aligned (none at the 256-byte
// aligned offsets pack_gt_raw gives); head and tail pixels are written by one thread each with
// three 2-byte stores, and a map at an odd address goes pixel by pixel in byte stores.  The
// gathers are 2-byte loads (neighbouring output pixels read neighbouring source pixels, so
// they hit the caches); the record, the scales and the inverse of the linear part are uniform
// over the workgroup.  Maps of different sizes share one launch: grid (x, image), x sized for
// the largest map, workgroups past a map's end leave at once.  Traffic is 6 bytes written and
// at most 6 read per pixel; no atomics, no LDS, no reduction: equal input gives equal bits.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "flow_sample.h"

#pragma clang fp contract(off)

using namespace oflow;

namespace {

constexpr int kGtaThreads = 256;

// How the flat pixel run of a map at byte address `addr` is cut: `head` single pixels, then
// `groups` groups of eight from a 16-byte boundary, then `tail` single pixels.
struct GtaCut {
  int head, tail;
  int64_t groups;
  __host__ __device__ int64_t threads() const { return groups + head + tail; }
};

__host__ __device__ inline GtaCut gta_cut(uint64_t addr, int64_t npix) {
  GtaCut c;
  if (addr & 1) {                                   // no 2-byte store is aligned: all single
    c.head = 0;
    c.groups = 0;
    c.tail = 0;
    return c;
  }
  // 6 p = -addr (mod 16)  <=>  3 p = -(addr / 2) (mod 8)  <=>  p = -3 (addr / 2) (mod 8)
  const int h = (int)((8 - (3 * ((addr >> 1) & 7)) % 8) % 8);
  c.head = (int)std::min<int64_t>(h, npix);
  c.groups = (npix - c.head) / 8;
  c.tail = (int)(npix - c.head - 8 * c.groups);
  return c;
}

__host__ __device__ inline int64_t gta_threads(uint64_t addr, int64_t npix) {
  return (addr & 1) ? npix : gta_cut(addr, npix).threads();
}

// What is uniform over a map: sizes, the record, pixel centre scales, inverse linear part.
struct GtaMap {
  const uint8_t* src;
  int h, w;
  float m[6];
  float fw, fh, imw, imh;
  float a00, a01, a10, a11, det;
  bool live;               // |det| >= 1e-12 (false for a NaN determinant)
  bool even;               // 2-byte loads are aligned
};

// An output pixel in three straight-line steps, so that a thread's eight gathers are all in
// flight before the first is used (a branch on a loaded B would put a wait between the pixels):
// where the source pixel lies (clamped into the map whatever the record, `inside` says whether
// it was there), its three samples, and what is written (0, 0, 0 when invalid).
__device__ __forceinline__ int gta_source(const GtaMap& g, int x, int y, bool& inside) {
  const float xc = __fdiv_rn(((float)x + 0.5f) * g.imw, g.fw);
  const float yc = __fdiv_rn(((float)y + 0.5f) * g.imh, g.fh);
  const float u = (g.m[0] * xc + g.m[1] * yc) + g.m[2];
  const float v = (g.m[3] * xc + g.m[4] * yc) + g.m[5];
  const float fx = floorf(u * g.fw), fy = floorf(v * g.fh);
  // every comparison is false for a NaN; an infinite u or v gives an infinite or NaN product
  inside = g.live && fx >= 0.f && fx < g.fw && fy >= 0.f && fy < g.fh;
  const int xs = (int)(inside ? fx : 0.f), ys = (int)(inside ? fy : 0.f);
  inside = inside && xs < g.w && ys < g.h;          // (float)w rounds up past 2^24
  return min(ys, g.h - 1) * g.w + min(xs, g.w - 1);   // h * w < 2^31
}

__device__ __forceinline__ void gta_load(const GtaMap& g, int p, unsigned& sr, unsigned& sg,
                                         unsigned& sb) {
  if (g.even) {
    const uint16_t* s16 = reinterpret_cast<const uint16_t*>(g.src) + 3 * (int64_t)p;
    sr = s16[0], sg = s16[1], sb = s16[2];
  } else {
    sr = ld16(g.src, 3 * (int64_t)p), sg = ld16(g.src, 3 * (int64_t)p + 1);
    sb = ld16(g.src, 3 * (int64_t)p + 2);
  }
}

__device__ __forceinline__ void gta_finish(const GtaMap& g, bool inside, unsigned sr, unsigned sg,
                                           unsigned sb, unsigned& R, unsigned& G, unsigned& B) {
  const float gx = __fdiv_rn((float)sr - 32768.f, 64.f), gy = __fdiv_rn((float)sg - 32768.f, 64.f);
  const float tx = __fdiv_rn(g.a11 * gx - g.a01 * gy, g.det);
  const float ty = __fdiv_rn(g.a00 * gy - g.a10 * gx, g.det);
  const float qx = rintf(tx * 64.f + 32768.f), qy = rintf(ty * 64.f + 32768.f);
  // outside the 16-bit range (or not a number): invalid, never clamped
  const bool valid = inside && sb != 0 && qx >= 0.f && qx <= 65535.f && qy >= 0.f && qy <= 65535.f;
  R = (unsigned)(valid ? qx : 0.f);
  G = (unsigned)(valid ? qy : 0.f);
  B = valid ? 1u : 0u;
}

// grid (x, n): thread t of image i owns group t (t < groups), else single pixel t - groups of
// the head and tail; thread 0 of workgroup 0 also copies the image's descriptor.
__global__ __launch_bounds__(kGtaThreads) void gt_augment_kernel(
    const uint8_t* __restrict__ raw, int64_t gt_bytes, int img_h, int img_w,
    const of_augment* __restrict__ params, uint8_t* __restrict__ out) {
  const int img = blockIdx.y;
  const of_image_desc d = reinterpret_cast<const of_image_desc*>(raw)[img];
  if (blockIdx.x == 0 && threadIdx.x == 0) reinterpret_cast<of_image_desc*>(out)[img] = d;
  if (d.h <= 0 || d.w <= 0) return;
  const int64_t npix = (int64_t)d.h * d.w;
  // a device descriptor that disagrees with the host's checked copy is never followed outside
  // the buffer
  if (d.offset < (int64_t)gridDim.y * (int64_t)sizeof(of_image_desc) ||
      d.offset > gt_bytes - 6 * npix)
    return;
  uint8_t* dst = out + d.offset;
  const bool odd = ((uintptr_t)dst & 1) != 0;
  const GtaCut cut = gta_cut((uintptr_t)dst, npix);
  const int64_t nthreads = odd ? npix : cut.threads();
  const int64_t t = (int64_t)blockIdx.x * kGtaThreads + threadIdx.x;
  if (t >= nthreads) return;

  const of_augment& a = params[img];
  GtaMap g;
  g.src = raw + d.offset;
  g.h = d.h;
  g.w = d.w;
  for (int k = 0; k < 6; ++k) g.m[k] = a.m[k];
  g.fw = (float)d.w;
  g.fh = (float)d.h;
  g.imw = (float)img_w;
  g.imh = (float)img_h;
  g.a00 = g.m[0] * g.imw;
  g.a01 = __fdiv_rn(g.m[1] * g.imh * g.fw, g.fh);
  g.a10 = __fdiv_rn(g.m[3] * g.imw * g.fh, g.fw);
  g.a11 = g.m[4] * g.imh;
  g.det = g.a00 * g.a11 - g.a01 * g.a10;
  g.live = fabsf(g.det) >= 1e-12f;
  g.even = ((uintptr_t)g.src & 1) == 0;

  if (!odd && t < cut.groups) {
    const int64_t p0 = cut.head + 8 * t;
    int y = (int)(p0 / d.w), x = (int)(p0 - (int64_t)y * d.w);
    int ps[8];
    bool in[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ps[j] = gta_source(g, x, y, in[j]);
      if (++x == d.w) { x = 0; ++y; }
    }
    unsigned s[24];
#pragma unroll
    for (int j = 0; j < 8; ++j) gta_load(g, ps[j], s[3 * j], s[3 * j + 1], s[3 * j + 2]);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      gta_finish(g, in[j], s[3 * j], s[3 * j + 1], s[3 * j + 2], s[3 * j], s[3 * j + 1],
                 s[3 * j + 2]);
    unsigned wd[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) wd[k] = s[2 * k] | (s[2 * k + 1] << 16);   // little-endian
    uint4* o4 = reinterpret_cast<uint4*>(dst + 6 * p0);
    o4[0] = make_uint4(wd[0], wd[1], wd[2], wd[3]);
    o4[1] = make_uint4(wd[4], wd[5], wd[6], wd[7]);
    o4[2] = make_uint4(wd[8], wd[9], wd[10], wd[11]);
    return;
  }
  // a single pixel: index i of the head and tail (every pixel of a map at an odd address)
  int64_t p = t;
  if (!odd) {
    const int64_t i = t - cut.groups;
    p = i < cut.head ? i : 8 * cut.groups + i;
  }
  const int y = (int)(p / d.w), x = (int)(p - (int64_t)y * d.w);
  bool in;
  const int ps = gta_source(g, x, y, in);
  unsigned R, G, B;
  gta_load(g, ps, R, G, B);
  gta_finish(g, in, R, G, B, R, G, B);
  if (!odd) {
    uint16_t* o16 = reinterpret_cast<uint16_t*>(dst + 6 * p);
    o16[0] = (uint16_t)R;
    o16[1] = (uint16_t)G;
    o16[2] = (uint16_t)B;
  } else {
    uint8_t* o8 = dst + 6 * p;
    o8[0] = (uint8_t)R, o8[1] = (uint8_t)(R >> 8);
    o8[2] = (uint8_t)G, o8[3] = (uint8_t)(G >> 8);
    o8[4] = (uint8_t)B, o8[5] = 0;
  }
}

}  // namespace

extern "C" {

int of_gt_augment(const void* dev_gt_raw, const of_image_desc* host_descs, int64_t gt_bytes, int n,
                  int img_h, int img_w, const of_augment* dev_params, void* dev_out,
                  void* stream) {
  OF_CHECK_ARG(dev_gt_raw && host_descs && dev_params && dev_out, "gt augment: null pointer");
  OF_CHECK_ARG(dev_out != dev_gt_raw, "gt augment: dev_out must not be dev_gt_raw");
  OF_CHECK_ARG((((uintptr_t)dev_gt_raw | (uintptr_t)dev_out) & 15) == 0,
               "gt augment: dev_gt_raw and dev_out must be 16-byte aligned");
  OF_CHECK_ARG(n >= 0 && n <= 65535, "gt augment: n outside 0..65535");
  OF_CHECK_ARG(img_h >= 1 && img_w >= 1, "gt augment: image size < 1");
  if (const int st = check_gt_descs("gt augment", host_descs, n, gt_bytes)) return st;
  OF_CHECK_ARG(n == 0 || gt_bytes > 0, "gt augment: gt_bytes must be the size of both buffers");
  if (n == 0) return OF_OK;
  int64_t most = 1;
  for (int i = 0; i < n; ++i)
    most = std::max(most, gta_threads((uint64_t)host_descs[i].offset,
                                      (int64_t)host_descs[i].h * host_descs[i].w));
  hipLaunchKernelGGL(gt_augment_kernel, dim3((unsigned)cdiv(most, kGtaThreads), (unsigned)n),
                     dim3(kGtaThreads), 0, as_stream(stream),
                     static_cast<const uint8_t*>(dev_gt_raw), gt_bytes, img_h, img_w, dev_params,
                     static_cast<uint8_t*>(dev_out));
  return check_launch("gt augment");
}

}  // extern "C"
