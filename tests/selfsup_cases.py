"""TEST INFRASTRUCTURE ONLY -- the seeded inputs that the host and the GPU tests of the
self-supervision kernels share (tests/test_selfsup_host.py checks on the CPU what the GPU tests
rely on: the restatement's own fp32 error and the share of near-kink cells, on these inputs).

n = 2 images per case.  Grids 7 x 9 (one partial block), 12 x 20 (240 cells: the tail of a
256-thread block) and 33 x 65 (2145 cells: several blocks, an odd tail past the block and the
wave, an odd total for the two-cell loads); the image is twice the grid.  Records: identity,
flip, zoom 1.3 with translation, rotation 5 degrees with zoom 1.05 (corners leave the frame),
all-zero m (degenerate)."""
from __future__ import annotations

import functools

import numpy as np

import selfsup_ref as R

N = 2
GRIDS = [(7, 9), (12, 20), (33, 65)]
RECORDS = ["identity", "flip", "zoom", "rot", "zero"]
CASES = [(g, r) for g in GRIDS for r in RECORDS]
IDS = ["%dx%d-%s" % (g + (r,)) for g, r in CASES]
# records whose exact map puts every cell centre on a cell centre of the teacher grid: the
# cells of the frame's border then sit ON the `inside` bound by construction
LATTICE = ("identity", "flip")


def records(name, H, W, colour=False):
    """The case's two records (the two zooms differ in strength and window position)."""
    col = [dict(gain=(1.6, 0.5, 1.2), brightness=-0.15, contrast=1.7, saturation=1.4, flags=1),
           dict(gain=(0.9, 1.1, 1.05), brightness=0.07, contrast=0.8, saturation=0.6, flags=1)] \
        if colour else [{}, {}]
    if name == "identity":
        recs = [R.zoom(H, W, 1.0, **col[0]), R.zoom(H, W, 1.0, **col[1])]
    elif name == "flip":
        recs = [R.zoom(H, W, 1.0, hflip=True, **col[0]), R.zoom(H, W, 1.0, hflip=True, **col[1])]
    elif name == "zoom":
        recs = [R.zoom(H, W, 1.3, 0.2, 0.9, **col[0]), R.zoom(H, W, 1.3, 0.7, 0.1, **col[1])]
    elif name == "rot":
        recs = [R.zoom(H, W, 1.05, deg=5.0, **col[0]),
                R.zoom(H, W, 1.05, deg=-5.0, hflip=True, **col[1])]
    else:
        assert name == "zero"
        recs = [R.record([0.0] * 6, **col[0]), R.record([0.0] * 6, **col[1])]
    return np.array(recs)


@functools.lru_cache(maxsize=None)
def case(grid, name):
    """Everything one case needs, computed once and shared (read-only): the float32 inputs, the
    float64 reference of the transform (plain and masked), the near-kink cells, and the distill
    inputs (the reference target and weight rounded to float32, a random student)."""
    fh, fw = grid
    H, W = 2 * fh, 2 * fw
    seed = 1000 * fh + 10 * fw + RECORDS.index(name)
    rng = np.random.default_rng(seed)
    recs = records(name, H, W)
    teacher = (rng.standard_normal((N, fh, fw, 2)) * 1.5).astype(np.float32)
    mask = rng.uniform(0.0, 1.0, (N, fh, fw)).astype(np.float32)
    mask[rng.uniform(size=mask.shape) < 0.2] = 0.0
    batch = rng.uniform(-0.5, 0.6, (N, H, W, 6)).astype(np.float32)
    target, weight = R.transform_flow(teacher, recs, (H, W))
    _, weight_m = R.transform_flow(teacher, recs, (H, W), mask)
    ik, vk = R.near_kink(teacher, recs, (H, W))
    student = (rng.standard_normal((N, fh, fw, 2)) * 1.5).astype(np.float32)
    out = dict(grid=grid, name=name, H=H, W=W, records=recs, teacher=teacher, mask=mask,
               batch=batch, target=target, weight=weight, weight_m=weight_m, inside_kink=ik,
               visible_kink=vk, student=student, dtarget=target.astype(np.float32),
               dweight=weight_m.astype(np.float32))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
