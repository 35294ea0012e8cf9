"""The image-coordinate warp convention as a CPU reference, built from oracle.ref_flow's own
sampler.  Not a test module: the warp-convention tests import it.

    x = j + flow[b,i,j,0] (column),  y = i + flow[b,i,j,1] (row),
    out[b,i,j] = bilinear_interpolation(f2[b], x, y)

with the grid formed in float32 exactly as oracle.ref_flow.warp_features forms its own
(transposed) one.  ``image_convention()`` puts it in place of oracle.ref_flow.warp_features for
the duration of a with-block: flow_module, photometric_loss, train_step and tests/census_ref.py
all call that module attribute, so the patched oracle is the whole-net, loss and census
reference of the image convention."""
import contextlib

import pytest
import torch

from oracle import ref_flow as R


def warp_features_image(flow, f2):
    _, h, w, _ = f2.shape
    ii, jj = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    grid = torch.stack([jj, ii], -1).to(torch.float32).unsqueeze(0)      # [column, row]
    pts = (grid + flow.to(torch.float32)).to(flow.dtype)
    return R.bilinear_interpolation(f2, pts)


@contextlib.contextmanager
def image_convention():
    mp = pytest.MonkeyPatch()
    mp.setattr(R, "warp_features", warp_features_image)
    try:
        yield
    finally:
        mp.undo()


def shifted_pair(h, w, dx, dy, seed=0, dtype=torch.float64):
    """(1, h, w, 6): image 2[y, x] = image 1[y + dy, x + dx], edge-replicated (as
    optical_flow_amd.data.synthetic_batch shifts, without its noise).  The true flow from
    image 1 to image 2 is (-dx, -dy) at full resolution."""
    g = torch.Generator().manual_seed(seed)
    img1 = torch.rand((h, w, 3), generator=g, dtype=torch.float64)
    ys = (torch.arange(h) + dy).clamp(0, h - 1)
    xs = (torch.arange(w) + dx).clamp(0, w - 1)
    img2 = img1[ys][:, xs]
    return torch.cat([img1, img2], -1).unsqueeze(0).to(dtype)


def true_flows(h, w, dx, dy, scales=4, dtype=torch.float64):
    """The constant true flow (-dx, -dy) / 2^(s+1) at h / 2^(s+1) x w / 2^(s+1), s < scales."""
    out = []
    for s in range(scales):
        k = 2 ** (s + 1)
        f = torch.empty((1, h // k, w // k, 2), dtype=dtype)
        f[..., 0] = -dx / k
        f[..., 1] = -dy / k
        out.append(f)
    return out


def interior_residuals(pair, flows, dx, dy):
    """Per scale, max |image 1 - warp(image 2, flow)| over the pixels at least
    |shift| / 2^(s+1) from each border, with whatever oracle.ref_flow.warp_features is."""
    H, W = pair.shape[1], pair.shape[2]
    res = []
    for s, f in enumerate(flows):
        k = 2 ** (s + 1)
        h, w = H // k, W // k
        r = R.resize_bilinear(pair, h, w)
        d = (r[..., :3] - R.warp_features(f, r[..., 3:])).abs()
        my, mx = abs(dy) // k, abs(dx) // k
        res.append(d[:, my:h - my, mx:w - mx].max().item())
    return res
