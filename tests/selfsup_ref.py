"""TEST INFRASTRUCTURE ONLY -- numpy restatements of the self-supervision kernels
(include/oflow.h: of_augment_batch, of_flow_transform, of_flow_distill_fwd), written from the
definitions.  Nothing in the product imports this module.

augment_batch_f32   of_augment_batch step by step in IEEE single arithmetic: the kernel is
                    checked against it bit for bit, as of_augment_pairs is against augment_np.
transform_flow      of_flow_transform in ``dtype`` (float64 is the reference; float32 shows how
                    far the same formulas in single precision lie from it).
near_kink           the cells whose inside / visible decision no finite precision can be held
                    to: one of the eight comparisons within KINK of its bound in float64.
distill             of_flow_distill_fwd's value S and d S / d student in ``dtype``.
The analytic image pair at the end turns a target into a photometric residual.
"""
from __future__ import annotations

import math

import numpy as np

from augment_np import AUGMENT_DTYPE, F32, IMAGE_MEANS, _axis, identity, record  # noqa: F401

KINK = 1e-3          # cells


# ---------------------------------------------------------------- records of the tests ----
def flip(h, w):
    return record([-1.0 / w, 0.0, 1.0, 0.0, 1.0 / h, 0.0])


def zoom(h, w, z, tx=0.5, ty=0.5, hflip=False, deg=0.0, **colour):
    """data_reader.sample_augment's map for one draw: zoom z, window position (tx, ty), flip,
    rotation by deg about the centre."""
    W, H = float(w), float(h)
    sgn = -1.0 if hflip else 1.0
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    a00, a01, a10, a11 = c * sgn / z, -s / z, s * sgn / z, c / z
    cx = W / (2 * z) + tx * (W * (1 - 1 / z))
    cy = H / (2 * z) + ty * (H * (1 - 1 / z))
    a02 = a00 * (-W / 2) + a01 * (-H / 2) + cx
    a12 = a10 * (-W / 2) + a11 * (-H / 2) + cy
    return record([a00 / W, a01 / W, a02 / W, a10 / H, a11 / H, a12 / H], **colour)


def zero():
    return record([0.0] * 6)


# ------------------------------------------------------------------- of_augment_batch ----
def augment_batch_f32(batch: np.ndarray, records) -> np.ndarray:
    """(n, h, w, 6) float32 + n records -> (n, h, w, 6) float32, every step an IEEE single
    operation in the order include/oflow.h states."""
    assert batch.dtype == F32
    n, h, w, _ = batch.shape
    records = np.asarray(records)
    assert records.shape == (n,)
    out = np.empty_like(batch)
    xc = (np.arange(w, dtype=F32) + F32(0.5))[None, :]
    yc = (np.arange(h, dtype=F32) + F32(0.5))[:, None]
    for b in range(n):
        rec = records[b]
        m = np.asarray(rec["m"], F32)
        u = (m[0] * xc + m[1] * yc) + m[2]
        v = (m[3] * xc + m[4] * yc) + m[5]
        assert u.dtype == F32 and v.dtype == F32
        x0, x1, fx = _axis(u * F32(w) - F32(0.5), w)
        y0, y1, fy = _axis(v * F32(h) - F32(0.5), h)
        src = batch[b]
        p00, p01, p10, p11 = src[y0, x0], src[y0, x1], src[y1, x0], src[y1, x1]
        fx3, fy3 = fx[..., None], fy[..., None]
        top = p00 + (p01 - p00) * fx3
        bot = p10 + (p11 - p10) * fx3
        x = top + (bot - top) * fy3
        assert x.dtype == F32
        if int(rec["flags"]) & 1:
            for k in range(2):
                val = (x[..., 3 * k:3 * k + 3].astype(np.float64) + IMAGE_MEANS).astype(F32)
                val = val * np.asarray(rec["gain"], F32)[None, None, :]
                val = val + F32(rec["brightness"])
                val = (val - F32(0.5)) * F32(rec["contrast"]) + F32(0.5)
                gray = (F32(0.114) * val[..., 0] + F32(0.587) * val[..., 1]) + \
                    F32(0.299) * val[..., 2]
                gray = gray[..., None]
                val = gray + (val - gray) * F32(rec["saturation"])
                val = np.minimum(np.maximum(val, F32(0.0)), F32(1.0))
                assert val.dtype == F32
                x[..., 3 * k:3 * k + 3] = (val.astype(np.float64) - IMAGE_MEANS).astype(F32)
        out[b] = x
    return out


# ------------------------------------------------------------------ of_flow_transform ----
def _taps(s, size, T):
    s = np.minimum(np.maximum(s, T(0)), T(size - 1))
    i0 = np.minimum(np.floor(s).astype(np.int64), size - 1)
    i1 = np.minimum(i0 + 1, size - 1)
    return i0, i1, (s - i0.astype(T)).astype(T)


def _bilerp(a, y0, y1, x0, x1, fx, fy):
    if a.ndim == 3:
        fx, fy = fx[..., None], fy[..., None]
    top = a[y0, x0] + (a[y0, x1] - a[y0, x0]) * fx
    bot = a[y1, x0] + (a[y1, x1] - a[y1, x0]) * fx
    return top + (bot - top) * fy


def _cells(rec, fh, fw, img_hw, T):
    """(px, py) of every student cell on the teacher grid, and the map's linear part A."""
    H, W = img_hw
    m = np.asarray(rec["m"]).astype(T)
    xc = ((np.arange(fw).astype(T) + T(0.5)) * T(W) / T(fw))[None, :]
    yc = ((np.arange(fh).astype(T) + T(0.5)) * T(H) / T(fh))[:, None]
    u = (m[0] * xc + m[1] * yc) + m[2]
    v = (m[3] * xc + m[4] * yc) + m[5]
    px, py = u * T(fw) - T(0.5), v * T(fh) - T(0.5)
    A = np.array([[m[0] * T(W), m[1] * T(H) * T(fw) / T(fh)],
                  [m[3] * T(W) * T(fh) / T(fw), m[4] * T(H)]], dtype=T)
    return px.astype(T), py.astype(T), A


def transform_flow(teacher, records, img_hw, mask=None, dtype=np.float64, parts=False):
    """teacher (n, fh, fw, 2), n records, optional mask (n, fh, fw) -> (target, weight) in
    ``dtype``.  ``parts``: also the per-image dict of px, py, t (for near_kink)."""
    T = dtype
    n, fh, fw, _ = teacher.shape
    records = np.asarray(records)
    assert records.shape == (n,)
    target = np.zeros((n, fh, fw, 2), T)
    weight = np.zeros((n, fh, fw), T)
    info = []
    for b in range(n):
        px, py, A = _cells(records[b], fh, fw, img_hw, T)
        x0, x1, fx = _taps(px, fw, T)
        y0, y1, fy = _taps(py, fh, T)
        t = _bilerp(teacher[b].astype(T), y0, y1, x0, x1, fx, fy)
        inside = (px >= 0) & (px <= fw - 1) & (py >= 0) & (py <= fh - 1)
        qx, qy = px + t[..., 0], py + t[..., 1]
        visible = (qx >= 0) & (qx <= fw - 1) & (qy >= 0) & (qy <= fh - 1)
        info.append({"px": px, "py": py, "qx": qx, "qy": qy})
        det = A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
        if not abs(det) >= 1e-12:
            continue                    # target and weight stay 0
        target[b, ..., 0] = (A[1, 1] * t[..., 0] - A[0, 1] * t[..., 1]) / det
        target[b, ..., 1] = (A[0, 0] * t[..., 1] - A[1, 0] * t[..., 0]) / det
        wm = np.ones((fh, fw), T) if mask is None else \
            _bilerp(mask[b].astype(T), y0, y1, x0, x1, fx, fy)
        weight[b] = np.where(inside & visible, wm, T(0))
    assert target.dtype == T and weight.dtype == T
    return (target, weight, info) if parts else (target, weight)


def near_kink(teacher, records, img_hw):
    """(inside_kink, visible_kink), each (n, fh, fw) bool: a cell whose px or py (its px + t.x
    or py + t.y) lies within KINK cells of one of its two bounds, in float64.  A degenerate
    record decides nothing by a comparison (its weight is 0 by the determinant): no kinks."""
    n, fh, fw, _ = teacher.shape
    _, _, info = transform_flow(teacher, records, img_hw, parts=True)
    ik = np.zeros((n, fh, fw), bool)
    vk = np.zeros((n, fh, fw), bool)
    for b in range(n):
        _, _, A = _cells(np.asarray(records)[b], fh, fw, img_hw, np.float64)
        if not abs(A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]) >= 1e-12:
            continue
        d = info[b]
        near = lambda v, hi: (np.abs(v) < KINK) | (np.abs(v - hi) < KINK)
        ik[b] = near(d["px"], fw - 1) | near(d["py"], fh - 1)
        vk[b] = near(d["qx"], fw - 1) | near(d["qy"], fh - 1)
    return ik, vk


def border_cells(fh, fw):
    b = np.zeros((fh, fw), bool)
    b[0], b[-1], b[:, 0], b[:, -1] = True, True, True, True
    return b


# --------------------------------------------------------------- of_flow_distill_fwd ----
def distill(student, target, weight, q, eps, dtype=np.float64):
    """(S, d S / d student): S = sum weight * (|s - t|^2 + eps^2)^(q/2); a cell of weight 0
    contributes exactly 0."""
    T = dtype
    e = student.astype(T) - target.astype(T)
    w = weight.astype(T)
    r2 = e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + T(eps) * T(eps)
    rho = np.sqrt(r2) if q == 1 else np.power(r2, T(q) / T(2))
    on = w != 0
    S = np.sum(np.where(on, w * rho, T(0)), dtype=T)
    g = np.where(on, w * (T(q) * rho / r2), T(0))[..., None] * e
    return S, g.astype(T)


# -------------------------------------------------------- the analytic image pair ----
# Two smooth images on continuous pixel-index coordinates with a known smooth flow between
# them: image 1 is image 2 read at (x, y) + flow(x, y), so the true flow warps image 2 onto
# image 1 exactly.
def analytic_flow(x, y, H, W):
    """A vector of 1 to 4 px, varying over the frame."""
    fx = 1.75 + 1.0 * np.sin(2 * np.pi * y / H + 0.3) * np.cos(np.pi * x / W)
    fy = -1.75 - 1.0 * np.cos(2 * np.pi * x / W - 0.2) * np.sin(np.pi * y / H + 0.4)
    return fx, fy


def image2(x, y, H, W):
    return (np.sin(2 * np.pi * 3.0 * x / W + 0.5) * np.cos(2 * np.pi * 2.0 * y / H) +
            0.5 * np.sin(2 * np.pi * (2.0 * x / W + 3.0 * y / H)))


def image1(x, y, H, W):
    fx, fy = analytic_flow(x, y, H, W)
    return image2(x + fx, y + fy, H, W)


def source_index(rec, xi, yi, H, W):
    """Pixel-index coordinates of the source of augmented pixel index (xi, yi)."""
    m = np.asarray(rec["m"], np.float64)
    u = (m[0] * (xi + 0.5) + m[1] * (yi + 0.5)) + m[2]
    v = (m[3] * (xi + 0.5) + m[4] * (yi + 0.5)) + m[5]
    return u * W - 0.5, v * H - 0.5


def teacher_of_analytic(fh, fw, H, W):
    """The true flow at the cell centres of a (fh, fw) grid, in cells: (1, fh, fw, 2)."""
    xi = ((np.arange(fw) + 0.5) * W / fw - 0.5)[None, :] + np.zeros((fh, 1))
    yi = ((np.arange(fh) + 0.5) * H / fh - 0.5)[:, None] + np.zeros((1, fw))
    fx, fy = analytic_flow(xi, yi, H, W)
    return np.stack([fx * fw / W, fy * fh / H], -1)[None]


def photometric_residual(rec, flow_cells, weight, H, W):
    """Mean over the cells of weight > 0 of |image1' - image2' warped by flow_cells|, the
    images augmented by ``rec`` (read analytically at the source position), at the cell centres
    of the (fh, fw) grid of ``flow_cells`` (fh, fw, 2)."""
    fh, fw = flow_cells.shape[:2]
    xi = ((np.arange(fw) + 0.5) * W / fw - 0.5)[None, :] + np.zeros((fh, 1))
    yi = ((np.arange(fh) + 0.5) * H / fh - 0.5)[:, None] + np.zeros((1, fw))
    a = image1(*source_index(rec, xi, yi, H, W), H, W)
    b = image2(*source_index(rec, xi + flow_cells[..., 0] * W / fw,
                             yi + flow_cells[..., 1] * H / fh, H, W), H, W)
    on = weight > 0
    assert on.any()
    return float(np.abs(a - b)[on].mean())
