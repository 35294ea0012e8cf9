"""The inputs of the SSIM GPU tests (tests/test_gpu_ssim.py), built on the CPU so that
tests/test_ssim_host.py can state their conditioning (S in [-1,1]; float32 against float64)
without a GPU.  Not a test module."""
import contextlib
import functools

import torch

import ssim_ref
from helpers import f64, rng_tensor
from warp_image_ref import image_convention

N = 3
# no window / one window / a single column of centres / one row of centres wider than a tile /
# a partial tile / tile edges crossed both ways (two-pixel halo, edge centres counted once)
LEVELS = [(1, 1), (3, 3), (5, 3), (3, 40), (13, 21), (40, 57)]
LOW_LEVELS = [(13, 21), (40, 57)]
# The low-texture images are 0.8 + 0.003 U with flows of 0.4 px.  With 0.8 + 0.002 U the
# float32 evaluation of the REFERENCE is 1.0e-5 (value) but 1.1e-4 to 1.2e-4 (d(flow)) from
# float64 at either flow scale -- its deviations y - my carry the rounding of numbers near 0.8,
# 6e-8 on 6e-4 -- which is over the REL_TOL / 10 that tests/test_ssim_host.py asks of every
# input; that error scales with base / amplitude, so the amplitude is the input changed.
LOW_AMPLITUDE = 0.003
LOW_FLOW_SCALE = 0.4
CONVENTIONS = ["reference", "image"]


def convention(cv):
    """The oracle's warp in convention ``cv`` for the duration of a with-block."""
    return image_convention() if cv == "image" else contextlib.nullcontext()


def textured():
    """Per level (images, flows): uniform images, flows of scale 3 (many samples clamp), as
    the census tests draw theirs."""
    flows = [rng_tensor((N, h, w, 2), 300 + i, scale=3.0) for i, (h, w) in enumerate(LEVELS)]
    imgs = [rng_tensor((N, h, w, 6), 400 + i, lo=-0.5, hi=0.6) for i, (h, w) in enumerate(LEVELS)]
    return imgs, flows


def low_texture():
    """Intensities 0.8 + LOW_AMPLITUDE U: the case an uncentred variance E[x^2] - mu^2 fails in
    float32 (sigma ~ 7e-7 beside mu^2 ~ 0.64)."""
    mean = torch.tensor(ssim_ref.MEANS + ssim_ref.MEANS, dtype=torch.float32)
    imgs = [0.8 + LOW_AMPLITUDE * rng_tensor((N, h, w, 6), 500 + i, lo=0.0, hi=1.0) - mean
            for i, (h, w) in enumerate(LOW_LEVELS)]
    flows = [rng_tensor((N, h, w, 2), 520 + i, scale=LOW_FLOW_SCALE)
             for i, (h, w) in enumerate(LOW_LEVELS)]
    return imgs, flows


def random_weights(levels=LEVELS):
    """Non-negative weights with exact zeros, on every pixel (so also on the centres that a
    neighbouring tile holds in its halo)."""
    out = []
    for i, (h, w) in enumerate(levels):
        u = rng_tensor((N, h, w), 600 + i, lo=-0.3, hi=1.5)
        out.append(u.clamp_min(0.0))
    return out


@functools.lru_cache(maxsize=None)
def level_reference(kind, cv, weighted=False):
    """Float64 reference of the ABI cases: per level (SSIM_l, d SSIM_l / d flow)."""
    imgs, flows = textured() if kind == "textured" else low_texture()
    levels = LEVELS if kind == "textured" else LOW_LEVELS
    wts = random_weights(levels) if weighted else [None] * len(levels)
    return [level_value_grad(f64(im), f64(f), cv, None if m is None else f64(m))
            for im, f, m in zip(imgs, flows, wts)]


def level_value_grad(img6, flow, cv, m=None):
    """(SSIM_l, d SSIM_l / d flow) of one level in the dtype of the inputs."""
    fo = flow.detach().clone().requires_grad_(True)
    with convention(cv):
        s = ssim_ref.level_sum(*ssim_ref.intensities(img6, fo), m)
    g = torch.autograd.grad(s, fo)[0] if s.requires_grad else torch.zeros_like(fo)
    return s.item(), g


# ------------------------------------------------------------------ pyramid cases ----
PYRAMID = (2, 64, 128)


def pyramid_case(levels):
    """(batch, flows) at 64 x 128, B = 2; with five levels the fifth, 2 x 4, has no window."""
    from optical_flow_amd.data import synthetic_batch
    n, H, W = PYRAMID
    batch = torch.from_numpy(synthetic_batch(n, H, W, seed=5))
    flows = [rng_tensor((n, H >> (s + 1), W >> (s + 1), 2), 50 + s, scale=2.0)
             for s in range(levels)]
    return batch, flows
