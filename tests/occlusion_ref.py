"""Occlusion masks and the weighted data terms restated from their definitions (DESIGN.md
"Occlusion masks"; include/oflow.h of_occ_mask_multi and the `_w` entry points), in whatever
dtype the inputs have (float64 in the tests), image convention only:

    x = j + f0, y = i + f1      (formed in float32, as oracle.ref_flow forms its grid)
    border: 0 <= x <= w-1 and 0 <= y <= h-1
    fb:     border and |f + g~|^2 <= alpha1 (|f|^2 + |g~|^2) + alpha2_l,
            g~ = bilinear_interpolation(partner's flow, (x, y)),  partner = (b + n/2) % n
    alpha2_l = alpha2 / 4^(l+1)  for level l of a pyramid

    photometric_w = (1/L) sum_l (1/(n h w 3)) sum_p w[p] sum_c |img1[p,c] - warped[p,c]|
    C_l           = (1/K) sum_p w[p] sum_o phi(e[p,o])      (census_ref's e, phi, K)

built from oracle.ref_flow.bilinear_interpolation, tests/warp_image_ref.py and
tests/census_ref.py.  Not a test module: the occlusion tests import it."""
import torch

import census_ref
from oracle import ref_flow as R
from warp_image_ref import image_convention, warp_features_image


def sample_points(flow):
    """(x, y) of every pixel, each (n,h,w): the float32 sum oracle.ref_flow's warp forms."""
    _, h, w, _ = flow.shape
    ii, jj = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    grid = torch.stack([jj, ii], -1).to(torch.float32).unsqueeze(0)
    pts = (grid + flow.to(torch.float32)).to(flow.dtype)
    return pts[..., 0], pts[..., 1]


def border(flow):
    """(mask, margin): margin is the distance of the sample point to the nearest of the four
    frame lines x = 0, x = w-1, y = 0, y = h-1 (the decision's margin)."""
    _, h, w, _ = flow.shape
    x, y = sample_points(flow)
    mask = (x >= 0) & (x <= w - 1) & (y >= 0) & (y <= h - 1)
    margin = torch.stack([x.abs(), (x - (w - 1)).abs(), y.abs(), (y - (h - 1)).abs()]).amin(0)
    return mask.to(flow.dtype), margin


def fb(flow, alpha1, alpha2_level):
    """(mask, border margin, lhs, rhs) of a doubled batch [forward ; swapped]."""
    n = flow.shape[0]
    assert n % 2 == 0
    partner = torch.roll(flow, -(n // 2), 0)            # image b reads (b + n/2) % n
    g = warp_features_image(flow, partner)
    lhs = ((flow + g) ** 2).sum(-1)
    rhs = alpha1 * ((flow ** 2).sum(-1) + (g ** 2).sum(-1)) + alpha2_level
    bm, margin = border(flow)
    return bm * (lhs <= rhs).to(flow.dtype), margin, lhs, rhs


def near(flow, mode, alpha1=0.01, alpha2_level=0.0, tol=1e-4):
    """The pixels whose decision margin is near zero: their mask may legitimately differ
    between two roundings."""
    if mode == "border":
        return border(flow)[1] < tol
    _, margin, lhs, rhs = fb(flow, alpha1, alpha2_level)
    return (margin < tol) | ((lhs - rhs).abs() < tol * (1 + rhs))


def masks(flows, mode, alpha1=0.01, alpha2=0.5):
    """ops.occlusion_masks: per pyramid level a (n,h,w) mask of 0.0 / 1.0."""
    if mode == "border":
        return [border(f)[0] for f in flows]
    return [fb(f, alpha1, alpha2 / 4.0 ** (s + 1))[0] for s, f in enumerate(flows)]


def photo_level(img6, flow, w=None):
    """sum_p w[p] sum_c |img1 - warped| of one level."""
    d = (img6[..., :3] - warp_features_image(flow, img6[..., 3:])).abs().sum(-1)
    return (d if w is None else w * d).sum()


def photometric(batch, flows, weights=None):
    H, W = batch.shape[1], batch.shape[2]
    total = batch.new_zeros(())
    for s, f in enumerate(flows):
        n, h, w, _ = f.shape
        assert h == int(H / 2.0 ** (s + 1)) and w == int(W / 2.0 ** (s + 1))
        r = R.resize_bilinear(batch, h, w)
        total = total + photo_level(r, f, None if weights is None else weights[s]) / (n * h * w * 3)
    return total / len(flows)


def census_level(g1, u, w, r):
    """The definition: every centre pixel's window sum times the centre's weight."""
    _, h, wd = g1.shape
    total = g1.new_zeros(())
    for dy, dx, ys, xs in census_ref._pairs(h, wd, r):
        sy, sx = census_ref._shift(ys, dy), census_ref._shift(xs, dx)
        e = (census_ref.tau(g1[:, sy, sx] - g1[:, ys, xs]) -
             census_ref.tau(u[:, sy, sx] - u[:, ys, xs]))
        total = total + (w[:, ys, xs] * census_ref.phi(e)).sum()
    return total / ((2 * r + 1) ** 2 - 1)


def census_level_closed_form(g1, u, w, r):
    """(C_l, dC_l/du) by the closed form the kernel uses:
    dC_l/du[q] = (1/K) sum_o (w[q] + w[q+o]) phi'(e[q,o]) tau'(u[q+o] - u[q])."""
    _, h, wd = g1.shape
    K = (2 * r + 1) ** 2 - 1
    total = g1.new_zeros(())
    grad = torch.zeros_like(u)
    C_T, C_D = census_ref.C_T, census_ref.C_D
    for dy, dx, ys, xs in census_ref._pairs(h, wd, r):
        sy, sx = census_ref._shift(ys, dy), census_ref._shift(xs, dx)
        d2 = u[:, sy, sx] - u[:, ys, xs]
        e = census_ref.tau(g1[:, sy, sx] - g1[:, ys, xs]) - census_ref.tau(d2)
        total = total + (w[:, ys, xs] * census_ref.phi(e)).sum()
        dphi = 2 * C_D * e / (C_D + e * e) ** 2
        dtau = C_T / (C_T + d2 * d2) ** 1.5
        grad[:, ys, xs] += (w[:, ys, xs] + w[:, sy, sx]) / K * dphi * dtau
    return total / K, grad


def gray_pair(img6, flow):
    """census_ref.gray_pair with the warp in the image convention."""
    with image_convention():
        return census_ref.gray_pair(img6, flow)


def census(batch, flows, r=3, weights=None):
    H, W = batch.shape[1], batch.shape[2]
    total = batch.new_zeros(())
    for s, f in enumerate(flows):
        n, h, w, _ = f.shape
        assert h == int(H / 2.0 ** (s + 1)) and w == int(W / 2.0 ** (s + 1))
        g1, u = gray_pair(R.resize_bilinear(batch, h, w), f)
        wt = torch.ones_like(g1) if weights is None else weights[s]
        total = total + census_level(g1, u, wt, r) / (n * h * w)
    return total / len(flows)


# ------------------------------------------------- the inputs of the occlusion tests ----
# Shared by the GPU parity tests and by the host test that asserts their conditioning (few
# pixels near a decision, both mask values well represented) on this reference alone.
ABI_LEVELS = [(1, 1), (5, 3), (13, 21), (40, 57)]
ABI_N = 4                                   # B = 2: two pairs with different flows
ABI_ALPHA1, ABI_ALPHA2S = 0.01, [0.5, 0.125, 0.125, 0.125]
FLOW_SCALE = {"border": 3.0, "fb": 0.3}     # fb at scale 3 is < 1 % valid
LAYER_SIZE = {"border": (2, 64, 96), "fb": (4, 48, 80)}
LAYER_FLOW_SCALE = {"border": 2.0, "fb": 0.3}
LAYER_SEED = 50


def _rng_tensor(shape, seed, scale):
    import numpy as np
    return torch.tensor(np.random.default_rng(seed).standard_normal(shape) * scale,
                        dtype=torch.float32)


def abi_flows(mode):
    """float32 flows of the mask kernel's ABI test, one per ABI_LEVELS entry."""
    return [_rng_tensor((ABI_N, h, w, 2), 300 + h, FLOW_SCALE[mode]) for h, w in ABI_LEVELS]


def layer_case(mode):
    """(batch (n,H,W,6), four float32 flow levels) of the LossLayer parity test; for "fb" the
    batch is the doubled one [pairs ; swapped pairs]."""
    from optical_flow_amd.data import synthetic_batch
    n, H, W = LAYER_SIZE[mode]
    if mode == "fb":
        b = torch.from_numpy(synthetic_batch(n // 2, H, W, seed=5))
        batch = torch.cat([b, torch.cat([b[..., 3:], b[..., :3]], -1)], 0)
    else:
        batch = torch.from_numpy(synthetic_batch(n, H, W, seed=5))
    flows = [_rng_tensor((n, H >> (s + 1), W >> (s + 1), 2), LAYER_SEED + s,
                         LAYER_FLOW_SCALE[mode]) for s in range(4)]
    return batch, [_condition(f, mode, 0.5 / 4.0 ** (s + 1)) for s, f in enumerate(flows)]


def _condition(flow, mode, alpha2_level, tol=1e-3):
    """The loss-parity flows must have no pixel within ``tol`` of a mask decision (a flipped
    mask pixel would change the loss by more than the tolerance): move the flow of every
    such pixel a little (by a tenth and 0.013 px, so that a sample on a frame line leaves it
    too) until none is left.  Deterministic; a few rounds at most."""
    flow = flow.clone()
    for _ in range(50):
        nr = near(flow.double(), mode, 0.01, alpha2_level, tol)
        if not nr.any():
            return flow
        flow[nr] = flow[nr] * 0.9 + 0.013
    raise AssertionError("could not condition the flows")
