"""TEST INFRASTRUCTURE ONLY -- numpy restatements of of_gt_augment (include/oflow.h), written
from the definition.  Nothing in the product imports this module.

gt_augment_f32   step by step in IEEE single arithmetic, in the stated order: the kernel is
                 checked against it bit for bit, as of_augment_pairs is against augment_np.
gt_augment_f64   independent: float64 throughout, the nearest pixel by its own rounding, the
                 exact inverse of the linear part by numpy.linalg.  Returns what decides a
                 pixel too (u*w, v*h), so a test can leave out the pixels no finite precision
                 can be held to.

Per output pixel (x, y) of a map of h x w under a record drawn for an H x W image:
  1. xc = (x + 0.5) * W / w,  yc = (y + 0.5) * H / h
  2. u = (m0*xc + m1*yc) + m2,  v = (m3*xc + m4*yc) + m5
  3. xs = floor(u * w),  ys = floor(v * h); invalid outside the map or for a non-finite u, v
  4. invalid where the source pixel has B == 0;  g = (R - 32768) / 64, (G - 32768) / 64
  5. A = [[m0*W, m1*H*w/h], [m3*W*h/w, m4*H]],  det = A00*A11 - A01*A10;  |det| < 1e-12 or
     NaN: the whole map is invalid
  6. g' = ((A11*g.x - A01*g.y) / det, (A00*g.y - A10*g.x) / det)
  7. q = rint(g' * 64 + 32768); invalid if either lies outside [0, 65535]
  8. (q.x, q.y, 1) where valid, (0, 0, 0) elsewhere
"""
from __future__ import annotations

import numpy as np

from augment_np import AUGMENT_DTYPE, F32, identity, record  # noqa: F401
from selfsup_ref import flip, zero, zoom  # noqa: F401


def gt_augment_f32(rgb: np.ndarray, rec, img_hw) -> np.ndarray:
    """One (h, w, 3) uint16 map -> the augmented (h, w, 3) uint16 map, every step an IEEE single
    operation in the order include/oflow.h states."""
    assert rgb.dtype == np.uint16 and rgb.ndim == 3 and rgb.shape[2] == 3
    h, w = rgb.shape[:2]
    H, W = F32(img_hw[0]), F32(img_hw[1])
    fw, fh = F32(w), F32(h)
    m = np.asarray(rec["m"], F32)
    out = np.zeros_like(rgb)
    with np.errstate(all="ignore"):
        a00 = m[0] * W
        a01 = m[1] * H * fw / fh
        a10 = m[3] * W * fh / fw
        a11 = m[4] * H
        det = a00 * a11 - a01 * a10
        assert all(v.dtype == F32 for v in (a00, a01, a10, a11, det))
        if not abs(det) >= F32(1e-12):
            return out
        xc = ((np.arange(w, dtype=F32) + F32(0.5)) * W / fw)[None, :]
        yc = ((np.arange(h, dtype=F32) + F32(0.5)) * H / fh)[:, None]
        u = (m[0] * xc + m[1] * yc) + m[2]
        v = (m[3] * xc + m[4] * yc) + m[5]
        assert u.dtype == F32 and v.dtype == F32
        fx, fy = np.floor(u * fw), np.floor(v * fh)
        inside = (fx >= 0) & (fx < fw) & (fy >= 0) & (fy < fh)        # False for NaN
        xs = np.where(inside, fx, 0).astype(np.int64)
        ys = np.where(inside, fy, 0).astype(np.int64)
        inside &= (xs < w) & (ys < h)
        xs, ys = np.minimum(xs, w - 1), np.minimum(ys, h - 1)
        src = rgb[ys, xs]
        valid = inside & (src[..., 2] != 0)
        gx = (src[..., 0].astype(F32) - F32(32768.0)) / F32(64.0)
        gy = (src[..., 1].astype(F32) - F32(32768.0)) / F32(64.0)
        tx = (a11 * gx - a01 * gy) / det
        ty = (a00 * gy - a10 * gx) / det
        qx = np.rint(tx * F32(64.0) + F32(32768.0))
        qy = np.rint(ty * F32(64.0) + F32(32768.0))
        assert qx.dtype == F32 and qy.dtype == F32
        valid &= (qx >= 0) & (qx <= 65535) & (qy >= 0) & (qy <= 65535)
    out[..., 0] = np.where(valid, qx, 0).astype(np.uint16)
    out[..., 1] = np.where(valid, qy, 0).astype(np.uint16)
    out[..., 2] = valid
    return out


def gt_augment_f64(rgb: np.ndarray, rec, img_hw):
    """The same map in float64, written independently: (valid bool (h, w), vectors float64
    (h, w, 2) rounded to 1/64 px, su, sv) where su = u*w, sv = v*h are the real source
    coordinates whose floors pick the source pixel."""
    h, w = rgb.shape[:2]
    H, W = float(img_hw[0]), float(img_hw[1])
    m = np.asarray(rec["m"], np.float64)
    ys_, xs_ = np.mgrid[0:h, 0:w]
    cx, cy = (xs_ + 0.5) * W / w, (ys_ + 0.5) * H / h
    with np.errstate(all="ignore"):
        su = (m[0] * cx + m[1] * cy + m[2]) * w
        sv = (m[3] * cx + m[4] * cy + m[5]) * h
        A = np.array([[m[0] * W, m[1] * H * w / h], [m[3] * W * h / w, m[4] * H]])
        det = np.linalg.det(A) if np.isfinite(A).all() else float("nan")
        valid = np.zeros((h, w), bool)
        vec = np.zeros((h, w, 2))
        if not abs(det) >= 1e-12:
            return valid, vec, su, sv
        ok = np.isfinite(su) & np.isfinite(sv) & (su >= 0) & (su < w) & (sv >= 0) & (sv < h)
        xi = np.clip(np.floor(np.where(ok, su, 0)), 0, w - 1).astype(np.int64)
        yi = np.clip(np.floor(np.where(ok, sv, 0)), 0, h - 1).astype(np.int64)
        src = rgb[yi, xi].astype(np.float64)
        g = (src[..., :2] - 32768.0) / 64.0
        gp = g @ np.linalg.inv(A).T
        q = np.rint(gp * 64.0 + 32768.0)
        valid = ok & (src[..., 2] != 0) & (q >= 0).all(-1) & (q <= 65535).all(-1)
        vec = np.where(valid[..., None], (q - 32768.0) / 64.0, 0.0)
    return valid, vec, su, sv


def decode(rgb: np.ndarray):
    """(valid bool, vectors float64) of a (h, w, 3) uint16 map: the devkit's decode."""
    return rgb[..., 2] != 0, (rgb[..., :2].astype(np.float64) - 32768.0) / 64.0


def make_map(h, w, rng, keep=0.3, mag=40.0):
    """A sparse (h, w, 3) uint16 map: about ``keep`` of the pixels valid (B is 1, or another
    non-zero value as KITTI's files never hold but the format allows), vectors uniform in
    +-mag px on the 1/64 grid, R and G of the invalid pixels left non-zero so that a kernel
    that forgets the flag is caught."""
    rgb = np.empty((h, w, 3), np.uint16)
    rgb[..., :2] = np.rint(rng.uniform(-mag, mag, (h, w, 2)) * 64.0 + 32768.0).astype(np.uint16)
    valid = rng.uniform(size=(h, w)) < keep
    rgb[..., 2] = np.where(valid, rng.choice([1, 1, 1, 7, 65535], (h, w)), 0)
    return rgb


# the maps and records of the tests: made once per session and never modified
SIZES = ((9, 14), (7, 12), (37, 83))
IMG_HW = (16, 32)
_cache = {}


def maps():
    """One map of each of SIZES."""
    if "maps" not in _cache:
        rng = np.random.default_rng(31)
        _cache["maps"] = [make_map(h, w, rng) for h, w in SIZES]
    return _cache["maps"]


def preset_opts():
    from optical_flow_amd.data_reader import AugmentOpts
    from optical_flow_amd.train import AUGMENT_PRESET
    return AugmentOpts(**AUGMENT_PRESET)


def record_sets():
    """{name: (3,) AUGMENT_DTYPE array, one record per map of SIZES} for an IMG_HW image: the
    identity, a flip, zoom 1.3 with an off-centre window, a 10 degree rotation, and two seeded
    sample_augment draws from the train command's preset."""
    if "records" not in _cache:
        from optical_flow_amd.data_reader import sample_augment
        H, W = IMG_HW
        sets = {"identity": [identity(H, W)] * 3, "flip": [flip(H, W)] * 3,
                "zoom": [zoom(H, W, 1.3, tx=0.3, ty=0.8)] * 3,
                "rotate": [zoom(H, W, 1.0, deg=10.0)] * 3}
        out = {k: np.array(v, AUGMENT_DTYPE) for k, v in sets.items()}
        for seed in (1, 2):
            out["preset%d" % seed] = sample_augment(preset_opts(), 3, H, W, seed, 0)
        _cache["records"] = out
    return _cache["records"]


def reference(name):
    """gt_augment_f32 of maps() under record_sets()[name], computed once per session."""
    key = ("ref", name)
    if key not in _cache:
        recs = record_sets()[name]
        _cache[key] = [gt_augment_f32(m, recs[i], IMG_HW) for i, m in enumerate(maps())]
    return _cache[key]
