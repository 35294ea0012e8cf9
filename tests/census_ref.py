"""The soft ternary census term restated from its definition (DESIGN.md "Census term";
include/oflow.h of_census_fwd_multi), in whatever dtype the inputs have (float64 in the tests):

    S = 255, c_t = 0.81, c_d = 0.1, r in {1,2,3}, K = (2r+1)^2 - 1
    g1[p]  = S * mean_{c<3} img6[p,c]
    u[p]   = S * mean_{c<3} warp(img6[...,3:6], f)[p,c]
    tau(d) = d / sqrt(c_t + d^2),   phi(e) = e^2 / (c_d + e^2)
    e[p,o] = tau(g1[p+o] - g1[p]) - tau(u[p+o] - u[p])   (o != 0, p+o inside the same image)
    C_l    = (1/K) sum_p sum_o phi(e[p,o]),   census = (1/L) sum_l C_l / (n h_l w_l)

with oracle.ref_flow's warp and resize.  Not a test module: the census tests import it."""
import torch

from oracle import ref_flow as R

S, C_T, C_D = 255.0, 0.81, 0.1


def tau(d):
    return d / torch.sqrt(C_T + d * d)


def phi(e):
    return e * e / (C_D + e * e)


def gray_pair(img6, flow):
    """(g1, u) of one level, each (n,h,w)."""
    g1 = S * img6[..., :3].mean(-1)
    u = S * R.warp_features(flow, img6[..., 3:]).mean(-1)
    return g1, u


def _pairs(h, w, r):
    """(dy, dx, rows of p, columns of p) of every offset that has a pair in an h x w image."""
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if (dy == 0 and dx == 0) or abs(dy) >= h or abs(dx) >= w:
                continue
            yield dy, dx, slice(max(0, -dy), h - max(0, dy)), slice(max(0, -dx), w - max(0, dx))


def _shift(s, d):
    return slice(s.start + d, s.stop + d)


def level_sum(g1, u, r):
    """C_l from (n,h,w) g1 and u.  Slicing within an image: no pair crosses a row end or an
    image boundary."""
    _, h, w = g1.shape
    total = g1.new_zeros(())
    for dy, dx, ys, xs in _pairs(h, w, r):
        e = (tau(g1[:, _shift(ys, dy), _shift(xs, dx)] - g1[:, ys, xs]) -
             tau(u[:, _shift(ys, dy), _shift(xs, dx)] - u[:, ys, xs]))
        total = total + phi(e).sum()
    return total / ((2 * r + 1) ** 2 - 1)


def level_closed_form(g1, u, r):
    """(C_l, dC_l/du) by the closed form the kernel uses: every unordered pair appears twice
    with the same value, so dC_l/du[q] = (2/K) sum_o phi'(e[q,o]) tau'(u[q+o] - u[q])."""
    _, h, w = g1.shape
    K = (2 * r + 1) ** 2 - 1
    total = g1.new_zeros(())
    grad = torch.zeros_like(u)
    for dy, dx, ys, xs in _pairs(h, w, r):
        d2 = u[:, _shift(ys, dy), _shift(xs, dx)] - u[:, ys, xs]
        e = tau(g1[:, _shift(ys, dy), _shift(xs, dx)] - g1[:, ys, xs]) - tau(d2)
        total = total + phi(e).sum()
        dphi = 2 * C_D * e / (C_D + e * e) ** 2
        dtau = C_T / (C_T + d2 * d2) ** 1.5
        grad[:, ys, xs] += (2.0 / K) * dphi * dtau
    return total / K, grad


def census(batch, flows, r=3):
    """The census term of a (n,H,W,6) batch and its flow pyramid (flows[s] at H/2^(s+1))."""
    H, W = batch.shape[1], batch.shape[2]
    total = batch.new_zeros(())
    for s, f in enumerate(flows):
        n, h, w, _ = f.shape
        assert h == int(H / 2.0 ** (s + 1)) and w == int(W / 2.0 ** (s + 1))
        g1, u = gray_pair(R.resize_bilinear(batch, h, w), f)
        total = total + level_sum(g1, u, r) / (n * h * w)
    return total / len(flows)
