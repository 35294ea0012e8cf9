"""The SSIM data term restated from its definition (DESIGN.md "SSIM term"; include/oflow.h
of_ssim_fwd_multi), in whatever dtype the inputs have (float64 in the tests):

    x = image 1 + mean_c,  y = warp(image 2, f) + mean_c,  mean = (123, 117, 104)/255
    per channel and interior centre p (1 <= i <= h-2, 1 <= j <= w-2), over p's 3 x 3 window:
    mx, my = means,  sx, sy, sxy = means of (x-mx)^2, (y-my)^2, (x-mx)(y-my)
    S = (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sx + sy + C2)),  C1 = 1e-4, C2 = 9e-4
    SSIM_l = sum_p m[p] sum_c (1 - S)/2,   ssim = (1/L) sum_l SSIM_l / (n (h_l-2)(w_l-2) 3)

with oracle.ref_flow's warp and resize (tests/warp_image_ref.image_convention() swaps the warp
for the image convention's, as for census_ref).  No clamp: S is in [-1,1] for any reals.  Also
the closed-form gradient the kernel uses.  Not a test module: the SSIM tests import it."""
import torch

from oracle import ref_flow as R

C1, C2 = 0.01 ** 2, 0.03 ** 2
MEANS = (123.0 / 255.0, 117.0 / 255.0, 104.0 / 255.0)


def intensities(img6, flow):
    """(x, y) of one level, each (n,h,w,3)."""
    mean = torch.tensor(MEANS, dtype=img6.dtype)
    return img6[..., :3] + mean, R.warp_features(flow, img6[..., 3:]) + mean


def _windows(t):
    """(9, n, h-2, w-2, c): the nine pixels of every window that lies inside the image."""
    h, w = t.shape[1], t.shape[2]
    return torch.stack([t[:, dy:h - 2 + dy, dx:w - 2 + dx] for dy in range(3) for dx in range(3)])


def window_stats(x, y):
    """mx, my, sx, sy, sxy per interior centre and channel (centred sums)."""
    wx, wy = _windows(x), _windows(y)
    mx, my = wx.mean(0), wy.mean(0)
    ex, ey = wx - mx, wy - my
    return mx, my, (ex * ex).mean(0), (ey * ey).mean(0), (ex * ey).mean(0)


def structural_similarity(x, y):
    """S per interior centre and channel, (n,h-2,w-2,3); h, w >= 3."""
    mx, my, sx, sy, sxy = window_stats(x, y)
    return ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sx + sy + C2))


def _centre_weights(m, like):
    return like.new_ones(like.shape[:3]) if m is None else m[:, 1:-1, 1:-1].to(like.dtype)


def level_sum(x, y, m=None):
    """SSIM_l from (n,h,w,3) x and y and optional (n,h,w) centre weights; 0 (no graph) for a
    level without a window."""
    if x.shape[1] < 3 or x.shape[2] < 3:
        return x.new_zeros(())
    d = (1 - structural_similarity(x, y)) / 2
    return (_centre_weights(m, d)[..., None] * d).sum()


def level_closed_form(x, y, m=None):
    """(SSIM_l, d SSIM_l / d y) by the closed form the kernel uses:
    d d_p / d y_q = (1/9) [P_p + Q_p (y_q - my_p) + R_p (x_q - mx_p)] for q in p's window,
    P = dd/dmy, Q = 2 dd/dsy, R = dd/dsxy, hence d SSIM_l / d y[q] = A_q + y_q B_q + x_q C_q
    with A, B, C the box sums of the per-centre coefficients over the centres that hold q."""
    n, h, w, _ = x.shape
    grad = torch.zeros_like(y)
    if h < 3 or w < 3:
        return x.new_zeros(()), grad
    mx, my, sx, sy, sxy = window_stats(x, y)
    a1, a2 = 2 * mx * my + C1, 2 * sxy + C2
    b1, b2 = mx * mx + my * my + C1, sx + sy + C2
    d = (1 - a1 * a2 / (b1 * b2)) / 2
    wt = _centre_weights(m, d)[..., None]
    P = -0.5 * (a2 / b2) * (2 * mx * b1 - a1 * 2 * my) / (b1 * b1)
    Q = a1 * a2 / (b1 * b2 * b2)
    Rc = -a1 / (b1 * b2)
    ka = wt * (P - Q * my - Rc * mx) / 9
    kb, kc = wt * Q / 9, wt * Rc / 9
    A, B, Cc = (torch.zeros_like(y) for _ in range(3))
    for dy in range(3):
        for dx in range(3):
            A[:, dy:h - 2 + dy, dx:w - 2 + dx] += ka
            B[:, dy:h - 2 + dy, dx:w - 2 + dx] += kb
            Cc[:, dy:h - 2 + dy, dx:w - 2 + dx] += kc
    return (wt * d).sum(), A + y * B + x * Cc


def level_coef(n, h, w, levels=1):
    """The normaliser of a level: 1 / (levels n (h-2)(w-2) 3), 0 without a window."""
    return 1.0 / (levels * n * (h - 2) * (w - 2) * 3) if h >= 3 and w >= 3 else 0.0


def ssim(batch, flows, weights=None):
    """The SSIM term of a (n,H,W,6) batch and its flow pyramid (flows[s] at H/2^(s+1));
    ``weights``: per level None or (n,h,w)."""
    H, W = batch.shape[1], batch.shape[2]
    total = batch.new_zeros(())
    for s, f in enumerate(flows):
        n, h, w, _ = f.shape
        assert h == int(H / 2.0 ** (s + 1)) and w == int(W / 2.0 ** (s + 1))
        x, y = intensities(R.resize_bilinear(batch, h, w), f)
        m = weights[s] if weights is not None else None
        total = total + level_sum(x, y, m) * level_coef(n, h, w)
    return total / len(flows)
