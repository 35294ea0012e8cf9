"""What the supervised loss term is checked against, none of it the project's own code: a torch
restatement on the CPU of the term's definition (include/oflow.h, of_supervised_fwd_multi),
float64 by default, its gradients from autograd; and the tests' inputs.

Per level l (flow F_l (n, fh, fw, 2) on its own grid) and image i with a KITTI map (gh, gw):
  u_l = the half-pixel bilinear upsampling with border replication of F_l[i] to (gh, gw), scaled
        by (gw / fw, gh / fh) (index arithmetic as kitti_flow_np.upsample_np),
  e = u_l - gt on the valid pixels (B != 0), gt = ((R, G) - 32768) / 64,
  rho = (e_x^2 + e_y^2 + eps^2)^(q/2),
  S_l,i = mean of rho over image i's valid pixels,
  S_l = mean of S_l,i over the images with a valid pixel (0 without one),
  term = sum_l lw_l S_l,  lw_l = 1 / L by default.
"""
import numpy as np
import torch

import kitti_flow_np as K


def _axis(g, n, like):
    s = np.clip((np.arange(g) + 0.5) * n / g - 0.5, 0.0, n - 1.0)       # float64, constants
    i0 = np.floor(s).astype(np.int64)
    return (torch.from_numpy(i0).to(like.device),
            torch.from_numpy(np.minimum(i0 + 1, n - 1)).to(like.device),
            torch.from_numpy(s - i0).to(like))


def upsample_t(f, gh, gw):
    """(fh, fw, 2) tensor on its own grid -> (gh, gw, 2) in pixels of the gh x gw image, of f's
    dtype, differentiable in f."""
    fh, fw = f.shape[:2]
    y0, y1, fy = _axis(gh, fh, f)
    x0, x1, fx = _axis(gw, fw, f)
    fx, fy = fx[None, :, None], fy[:, None, None]
    p00, p01 = f[y0][:, x0], f[y0][:, x1]
    p10, p11 = f[y1][:, x0], f[y1][:, x1]
    top = p00 + (p01 - p00) * fx
    bot = p10 + (p11 - p10) * fx
    val = top + (bot - top) * fy
    return val * torch.tensor([gw / fw, gh / fh], dtype=f.dtype, device=f.device)


def level_value(flow, maps, q, eps):
    """S_l of one level: ``flow`` (n, fh, fw, 2) tensor (any dtype and device), ``maps`` the
    first len(maps) images' ground truth (the others have none)."""
    per_image = []
    for i, rgb in enumerate(maps):
        valid = torch.from_numpy(np.asarray(rgb)[:, :, 2] != 0).to(flow.device)
        if not bool(valid.any()):
            continue
        gt = torch.from_numpy((np.asarray(rgb)[:, :, :2].astype(np.float64) - 32768.0) / 64.0)
        e = upsample_t(flow[i], rgb.shape[0], rgb.shape[1])[valid] - gt.to(flow)[valid]
        per_image.append(((e * e).sum(-1) + eps * eps).pow(q / 2.0).mean())
    if not per_image:
        return flow.sum() * 0.0
    return torch.stack(per_image).mean()


def supervised_ref(flows, maps, q=1.0, eps=0.01, level_weights=None, dtype=torch.float64):
    """(term, [S_l], [d term / d F_l]) as numpy float64; ``flows``: per level an (n, fh, fw, 2)
    array; evaluated in ``dtype``."""
    ts = [torch.tensor(np.asarray(f), dtype=dtype, requires_grad=True) for f in flows]
    lw = [1.0 / len(ts)] * len(ts) if level_weights is None else list(level_weights)
    vals = [level_value(t, maps, q, eps) for t in ts]
    term = sum(w * v for w, v in zip(lw, vals))
    grads = torch.autograd.grad(term, ts, allow_unused=True)
    grads = [np.zeros(t.shape) if g is None else g.double().numpy() for g, t in zip(grads, ts)]
    return float(term.detach()), [float(v.detach()) for v in vals], grads


# ---- inputs -----------------------------------------------------------------------------------
ERR = np.array([0.25, 1.0, 2.5, 3.5, 6.0, 20.0])     # none at 0: the penalty's kink at e = 0
#                                                      does not set the conditioning


def make_flow(fh, fw, gh, gw, rng):
    """A float32 (fh, fw, 2) flow on its own grid whose native magnitude is in [0, 48] px, with
    one direction +-0.2 rad."""
    mag = rng.uniform(0.0, 48.0, (fh, fw))
    ang = rng.uniform(0.0, 2 * np.pi) + rng.uniform(-0.2, 0.2, (fh, fw))
    native = np.stack([mag * np.cos(ang), mag * np.sin(ang)], -1)
    return (native * np.array([fw / gw, fh / gh])).astype(np.float32)


def make_gt(up, rng, keep=0.3):
    """A ground-truth map (h, w, 3) uint16 for the float64 native-size flow ``up``: about
    ``keep`` of the pixels valid, ground truth = up + an error vector of random direction whose
    magnitude is drawn from ERR, quantised to 1/64."""
    h, w = up.shape[:2]
    valid = rng.uniform(size=(h, w)) < keep
    m = rng.choice(ERR, (h, w))
    a = rng.uniform(0.0, 2 * np.pi, (h, w))
    q = np.rint((up + np.stack([m * np.cos(a), m * np.sin(a)], -1)) * 64.0) / 64.0
    rgb = np.zeros((h, w, 3), np.uint16)
    rgb[:, :, :2] = np.where(valid[:, :, None], np.clip(q * 64.0 + 32768.0, 0, 65535), 0)
    rgb[:, :, 2] = valid
    return rgb


def make_case(grids, sizes, seed):
    """One batch: per level of ``grids`` [(fh, fw), ...] a float32 flow (n, fh, fw, 2), and the n
    ground-truth maps of the given sizes, built around the first level's upsampled flow.  The
    coarser levels' flows are drawn on their own: their errors are whatever two independent
    fields of up to 48 px differ by."""
    rng = np.random.default_rng(seed)
    flows = [np.stack([make_flow(fh, fw, gh, gw, rng) for gh, gw in sizes]) for fh, fw in grids]
    maps = [make_gt(K.upsample_np(flows[0][i], gh, gw), rng) for i, (gh, gw) in enumerate(sizes)]
    return flows, maps


# name -> (grids, the batch's ground-truth sizes, seed): every input of tests/test_gpu_supervised.py
# that is compared with the restatement under a tolerance
CASES = {
    "three_sizes": ([(8, 16), (4, 8), (2, 4), (1, 2)], [(37, 61), (33, 67), (13, 21)], 21),
    "one_cell_grid": ([(1, 1)], [(5, 7)], 22),                    # every clamp active
    "one_pixel_map": ([(4, 4)], [(1, 1)], 23),
    "wide": ([(12, 20)], [(47, 125)], 24),
    "coarse_under_full": ([(3, 5)], [(375, 1242)], 25),           # > 10^5 pixels per cell
    "full_size": ([(96, 320), (48, 160), (24, 80), (12, 40)], [(375, 1242)] * 2, 26),
    "layer": ([(32, 64), (16, 32), (8, 16), (4, 8)], [(37, 61), (40, 125)], 27),
}
QS = (1.0, 0.4)
EPS = 0.01
_cache = {}


def case(name):
    """(flows, maps) of CASES[name], made once per session and never modified.  The 1 x 1
    map's one pixel is made valid (the draw leaves it invalid 70 % of the time)."""
    if name not in _cache:
        grids, sizes, seed = CASES[name]
        flows, maps = make_case(grids, sizes, seed)
        if name == "one_pixel_map":
            maps[0][0, 0, 2] = 1
            up = K.upsample_np(flows[0][0], 1, 1)[0, 0]
            maps[0][0, 0, :2] = np.rint((up + (2.5, 0.0)) * 64.0) + 32768
        _cache[name] = (flows, maps)
    return _cache[name]


def reference(name, q):
    """supervised_ref of a case in float64, computed once per session."""
    key = (name, q)
    if key not in _cache:
        flows, maps = case(name)
        _cache[key] = supervised_ref(flows, maps, q, EPS)
    return _cache[key]
