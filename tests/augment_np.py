"""TEST INFRASTRUCTURE ONLY -- numpy float32 restatement of of_augment_pairs (include/oflow.h),
written from the definition, step by step in the same IEEE single arithmetic, so the kernel is
checked bit for bit.  Nothing in the product imports this module.

Per output pixel (x, y) of pair b, for each of the pair's two images (own size sh x sw):
  1. xc = x + 0.5, yc = y + 0.5;  u = (m0*xc + m1*yc) + m2,  v = (m3*xc + m4*yc) + m5
  2. sx = u*sw - 0.5,  sy = v*sh - 0.5
  3. sx clamped to [0, sw-1], sy to [0, sh-1]
  4. x0 = floor(sx), x1 = min(x0+1, sw-1), fx = sx - x0; the same for y
  5. per channel on the 8-bit taps as float32: top = p00 + (p01-p00)*fx,
     bot = p10 + (p11-p10)*fx, val = top + (bot-top)*fy
  6. val = val / 255
  7. if flags & 1: val *= gain[c]; val += brightness; val = (val-0.5)*contrast + 0.5;
     gray = (0.114*B + 0.587*G) + 0.299*R of the three channels at that point;
     val = gray + (val-gray)*saturation; val = min(max(val, 0), 1)
  8. out = float32(float64(val) - mean[c])
  9. a frame with h <= 0 or w <= 0: val = 0 in step 8.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
IMAGE_MEANS = np.array([123.0, 117.0, 104.0]) / 255.0          # float64

AUGMENT_DTYPE = np.dtype([("m", np.float32, (6,)), ("gain", np.float32, (3,)),
                          ("brightness", np.float32), ("contrast", np.float32),
                          ("saturation", np.float32), ("flags", np.int32),
                          ("pad", np.int32, (3,))])


def record(m, gain=(1.0, 1.0, 1.0), brightness=0.0, contrast=1.0, saturation=1.0, flags=0):
    """One of_augment record (a 0-d structured value) from Python numbers."""
    r = np.zeros((), AUGMENT_DTYPE)
    r["m"] = np.asarray(m, np.float64).astype(F32)
    r["gain"] = np.asarray(gain, np.float64).astype(F32)
    r["brightness"], r["contrast"], r["saturation"] = brightness, contrast, saturation
    r["flags"] = flags
    return r


def identity(out_h: int, out_w: int):
    """The plain full-frame map, no colour stage."""
    return record([1.0 / out_w, 0.0, 0.0, 0.0, 1.0 / out_h, 0.0])


def _axis(s, size):
    s = np.minimum(np.maximum(s, F32(0.0)), F32(size - 1))
    i0 = np.floor(s).astype(np.int64)
    i1 = np.minimum(i0 + 1, size - 1)
    f = s - i0.astype(F32)
    assert f.dtype == F32
    return i0, i1, f


def augment_image(img: np.ndarray, out_h: int, out_w: int, rec) -> np.ndarray:
    """One 8-bit (h, w, 3) BGR frame -> (out_h, out_w, 3) float32, mean-subtracted."""
    out = np.empty((out_h, out_w, 3), F32)
    sh, sw = img.shape[:2]
    if sh <= 0 or sw <= 0:
        out[...] = (np.zeros(3, F32).astype(np.float64) - IMAGE_MEANS).astype(F32)
        return out
    m = np.asarray(rec["m"], F32)
    xc = (np.arange(out_w, dtype=F32) + F32(0.5))[None, :]
    yc = (np.arange(out_h, dtype=F32) + F32(0.5))[:, None]
    u = (m[0] * xc + m[1] * yc) + m[2]
    v = (m[3] * xc + m[4] * yc) + m[5]
    assert u.dtype == F32 and v.dtype == F32
    sx = u * F32(sw) - F32(0.5)
    sy = v * F32(sh) - F32(0.5)
    x0, x1, fx = _axis(sx, sw)
    y0, y1, fy = _axis(sy, sh)
    src = img.astype(F32)
    p00, p01 = src[y0, x0], src[y0, x1]                         # (out_h, out_w, 3)
    p10, p11 = src[y1, x0], src[y1, x1]
    fx3, fy3 = fx[..., None], fy[..., None]
    top = p00 + (p01 - p00) * fx3
    bot = p10 + (p11 - p10) * fx3
    val = top + (bot - top) * fy3
    val = val / F32(255.0)
    if int(rec["flags"]) & 1:
        val = val * np.asarray(rec["gain"], F32)[None, None, :]
        val = val + F32(rec["brightness"])
        val = (val - F32(0.5)) * F32(rec["contrast"]) + F32(0.5)
        gray = (F32(0.114) * val[..., 0] + F32(0.587) * val[..., 1]) + F32(0.299) * val[..., 2]
        gray = gray[..., None]
        val = gray + (val - gray) * F32(rec["saturation"])
        val = np.minimum(np.maximum(val, F32(0.0)), F32(1.0))
    assert val.dtype == F32
    out[...] = (val.astype(np.float64) - IMAGE_MEANS[None, None, :]).astype(F32)
    return out


def augment_pairs(frames, out_h: int, out_w: int, params) -> np.ndarray:
    """frames: [(img1_bgr_u8, img2_bgr_u8), ...] with swaps applied, params: one record per
    pair -> (B, out_h, out_w, 6) float32."""
    params = np.asarray(params)
    assert params.shape == (len(frames),)
    out = np.zeros((len(frames), out_h, out_w, 6), F32)
    for i, (a, b) in enumerate(frames):
        out[i, :, :, :3] = augment_image(a, out_h, out_w, params[i])
        out[i, :, :, 3:] = augment_image(b, out_h, out_w, params[i])
    return out
