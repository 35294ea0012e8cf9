"""The image-coordinate warp convention on the GPU (ops.warp(..., convention="image"), the _cv
entry points, FlowNet / LossLayer with warp_convention="image"):

    x = j + flow[b,i,j,0] (column),  y = i + flow[b,i,j,1] (row),  out = bilinear(inp, x, y)

against the float64 oracle with its warp replaced by tests/warp_image_ref.py (the oracle's own
sampler on the [column, row] grid).  All shapes but one are non-square: a transposition error
is invisible on a square with symmetric data.  Tolerance: the project's REL_TOL unless a test
says otherwise."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import census_ref
from helpers import REL_TOL, dev, f64, rel_inf, rel_l2, rng_tensor
from oracle import ref_flow as R
from test_gpu_smooth_loss import ref_smooth
from warp_image_ref import image_convention, shifted_pair, warp_features_image

pytestmark = pytest.mark.gpu

IMAGE = 1                                    # OF_WARP_IMAGE
SHAPES = [(2, 8, 12, 64),                    # gather form, w > h
          (1, 12, 8, 64),                    # gather form, h > w
          (1, 18, 35, 64),                   # ragged 4 x 4 tiles
          (1, 16, 16, 128),                  # two channel passes, square (asymmetric flows)
          (1, 6, 10, 4),                     # vec form
          (1, 5, 7, 3),                      # scalar form
          (2, 1, 9, 64),                     # degenerate row
          (1, 9, 1, 4)]                      # degenerate column
# the first six take mode A (R <= 8), the last the fixed-point path
FAMILIES = ["normal", "uniform6", "const", "integer", "outward", "converge", "uniform20"]
MODE_A = FAMILIES[:6]


def _off_integer(f):
    """Fractional parts moved into [2e-3, 1 - 2e-3]: grid + flow stays >= 1e-3 from an integer
    (the floor kink is not the subject)."""
    fl = torch.floor(f)
    return fl + (f - fl).clamp(2e-3, 1.0 - 2e-3)


def make_flow(family, shape, seed):
    n, h, w, _ = shape
    ii, jj = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
    if family == "normal":
        return _off_integer(rng_tensor((n, h, w, 2), seed, scale=0.3))
    if family == "uniform6":                 # the largest mode-A radius: floor(6 + 0.01) + 2 = 8
        f = _off_integer(rng_tensor((n, h, w, 2), seed, lo=-5.99, hi=5.99))
        f[0, 0, 0, 0] = 5.995
        return f
    if family == "const":
        return torch.tensor([3.25, -1.5]).expand(n, h, w, 2).contiguous()
    if family == "integer":                  # weights exactly 1 and 0
        r = np.random.default_rng(seed)
        return torch.tensor(r.integers(-3, 4, size=(n, h, w, 2)), dtype=torch.float32)
    if family == "outward":                  # every border band pushed out of frame, within +-6
        fx = 5.9 * (2.0 * (jj + 0.5) / w - 1.0)
        fy = 5.9 * (2.0 * (ii + 0.5) / h - 1.0)
        f = torch.stack([fx, fy], -1).expand(n, h, w, 2).contiguous()
        return _off_integer(f + rng_tensor((n, h, w, 2), seed, scale=0.05)).clamp(-5.99, 5.99)
    if family == "converge":                 # all pixels within 6 px of one pixel point at it
        ty, tx = h // 2, w // 2
        near = ((ii - ty).abs() <= 6) & ((jj - tx).abs() <= 6)
        f = torch.stack([tx - jj + 0.37, ty - ii + 0.41], -1)
        f = torch.where(near.unsqueeze(-1), f, torch.full_like(f, 0.25))
        return f.expand(n, h, w, 2).contiguous()
    assert family == "uniform20"
    f = _off_integer(rng_tensor((n, h, w, 2), seed, lo=-20.0, hi=20.0))
    f[0, 0, 0, 1] = -19.5                    # R > 8 whatever the draw
    return f


@functools.lru_cache(maxsize=None)
def case(si, family):
    """Inputs and the float64 reference of one (shape, family): the forward, and with the
    cotangent g the gradients d(inp), d(flow).  Computed once, shared, never modified."""
    shape = SHAPES[si]
    seed = 1000 + 10 * si + FAMILIES.index(family)
    inp = rng_tensor(shape, seed + 1)
    flow = make_flow(family, shape, seed + 2)
    g = rng_tensor(shape, seed + 3)
    a, fo = f64(inp).requires_grad_(True), f64(flow).requires_grad_(True)
    out = warp_features_image(fo, a)
    (out * f64(g)).sum().backward()
    return inp, flow, g, out.detach(), a.grad, fo.grad


ALL = [(si, fam) for si in range(len(SHAPES)) for fam in FAMILIES]
IDS = ["%s-%s" % ("x".join(map(str, SHAPES[si])), fam) for si, fam in ALL]


def _ops():
    from optical_flow_amd import ops
    return ops


def _lib():
    from optical_flow_amd import _lib
    return _lib.lib()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def _ptrs(ts):
    return _arr(C.c_void_p, [t.data_ptr() for t in ts])


# ------------------------------------------------------------------- 1. forward --------
@pytest.mark.parametrize("si,family", ALL, ids=IDS)
def test_forward(si, family):
    """Within REL_TOL of the reference, and BITWISE ops.bilinear(inp, grid + flow) with the
    [column, row] grid added in float32 on the device: the same tap arithmetic."""
    ops = _ops()
    inp, flow, _, out_ref, _, _ = case(si, family)
    n, h, w, c = SHAPES[si]
    di, df = dev(inp), dev(flow)
    out = ops.warp(di, df, convention="image")
    ii, jj = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"),
                            indexing="ij")
    grid = torch.stack([jj, ii], -1).to(torch.float32).unsqueeze(0)
    absolute = ops.bilinear(di, (grid + df).contiguous())
    torch.cuda.synchronize()
    assert rel_inf(out, out_ref) < REL_TOL
    assert torch.equal(out, absolute)


# ------------------------------------------------------------- 2. atomic backward ------
@pytest.mark.parametrize("si,family", ALL, ids=IDS)
def test_backward_atomic(si, family):
    """The float-atomic form (ops.set_deterministic(False)): d(inp) and d(flow) against float64
    autograd of the reference; and of_warp_bwd_cv with a dflow_add (padded rows, ld 4)."""
    from optical_flow_amd._lib import call
    ops = _ops()
    inp, flow, g, _, dinp_ref, dflow_ref = case(si, family)
    n, h, w, c = SHAPES[si]
    prev = ops.set_deterministic(False)
    try:
        ad, fd = dev(inp).requires_grad_(True), dev(flow).requires_grad_(True)
        (ops.warp(ad, fd, convention="image") * dev(g)).sum().backward()
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(prev)
    assert rel_inf(ad.grad, dinp_ref) < REL_TOL
    assert rel_inf(fd.grad, dflow_ref) < REL_TOL
    add = rng_tensor((n, h, w, 4), 77 + si)
    dg, di, dfl, dadd = dev(g), dev(inp), dev(flow), dev(add)
    dinp = torch.zeros(SHAPES[si], device="cuda")
    dflow = torch.full((n, h, w, 2), float("nan"), device="cuda")
    call("of_warp_bwd_cv", P(dg), P(di), n, h, w, c, P(dfl), P(dinp), P(dflow), P(dadd), 4,
         IMAGE, None)
    torch.cuda.synchronize()
    assert rel_inf(dinp, dinp_ref) < REL_TOL
    assert rel_inf(dflow, dflow_ref + f64(add)[..., :2]) < REL_TOL


# ------------------------------------------------------ 3. deterministic backward ------
def det_call(si, family, add=None):
    """of_warp_bwd_det_cv in the image convention -> (dinp, dflow, R, hits) with R and the
    mode-B hit count read from the workspace header."""
    from optical_flow_amd._lib import call
    lib = _lib()
    inp, flow, g, _, _, _ = case(si, family)
    n, h, w, c = SHAPES[si]
    wsb = lib.of_warp_bwd_det_workspace(n, h, w, c)
    hoff = lib.of_warp_bwd_det_header(n, h, w, c)
    dg, di, dfl = dev(g), dev(inp), dev(flow)
    ws = torch.full(((wsb + 3) // 4,), -7, dtype=torch.int32, device="cuda")
    dinp = torch.full(SHAPES[si], float("nan"), device="cuda")
    dflow = torch.full((n, h, w, 2), float("nan"), device="cuda")
    call("of_warp_bwd_det_cv", P(dg), P(di), n, h, w, c, P(dfl), P(dinp), P(dflow), P(add),
         4 if add is not None else 0, IMAGE, P(ws), wsb, None)
    torch.cuda.synchronize()
    hdr = ws[hoff // 4: hoff // 4 + 64 * 129].cpu()
    rr = max(int(hdr[64 * (33 + k)]) for k in range(32))
    found = int(sum(int(hdr[64 * (1 + k)]) for k in range(32)))
    det_call.overflowed = int(hdr[0])        # bins beyond TILE_CAP, left to the rest pass
    return dinp, dflow, rr, found


@pytest.mark.parametrize("si,family", ALL, ids=IDS)
def test_backward_deterministic(si, family):
    """of_warp_bwd_det_cv: the header reports mode A (R <= 8, no mode-B count) for the first
    six families and the fixed-point path for +-20; the 4 x 4 tiles with their rest pass (key
    34 = 2), the tiles inside the window kernel (1) and the per-destination scan (0) BITWISE
    equal, the two bin-overflow families included; the fixed-point result (key 28 = 0) within
    1e-5 of the window's; d(flow) bitwise equal across all paths; two calls bitwise equal;
    ops.warp under ops.deterministic() the same numbers."""
    ops = _ops()
    lib = _lib()
    inp, flow, g, _, dinp_ref, dflow_ref = case(si, family)
    n, h, w, c = SHAPES[si]
    res = {}
    try:
        for k34 in (2, 1, 0):
            assert lib.of_set_tuning(34, k34) == 0
            res[k34] = det_call(si, family)
            if k34 == 2 and SHAPES[si] == (1, 18, 35, 64) and family in ("outward", "converge"):
                assert det_call.overflowed > 0       # the overflow families do overflow a bin
        again = det_call(si, family)
        assert lib.of_set_tuning(34, 2) == 0
        assert lib.of_set_tuning(28, 0) == 0
        fixed = det_call(si, family)
    finally:
        lib.of_set_tuning(34, 2)
        lib.of_set_tuning(28, 8)
    dinp, dflow, rr, found = res[2]
    if family in MODE_A:
        assert rr <= 8 and found == 0, (rr, found)
    else:
        assert rr > 8 and found != 4 * n * h * w, (rr, found)
    assert rel_inf(dinp, dinp_ref) < REL_TOL
    assert rel_inf(dflow, dflow_ref) < REL_TOL
    for k34 in (1, 0):
        assert torch.equal(res[k34][0], dinp), k34
        assert torch.equal(res[k34][1], dflow), k34
    assert torch.equal(again[0], res[0][0]) and torch.equal(again[1], res[0][1])
    assert rel_inf(fixed[0], dinp_ref) < REL_TOL
    assert rel_inf(fixed[0], dinp) < 1e-5
    assert torch.equal(fixed[1], dflow)
    with ops.deterministic(True):
        ad, fd = dev(inp).requires_grad_(True), dev(flow).requires_grad_(True)
        (ops.warp(ad, fd, convention="image") * dev(g)).sum().backward()
        torch.cuda.synchronize()
    assert torch.equal(ad.grad, dinp) and torch.equal(fd.grad, dflow)


@pytest.mark.parametrize("si,family", [(0, "normal"), (2, "outward"), (5, "uniform6"),
                                       (3, "uniform20")])
def test_backward_deterministic_with_addend(si, family):
    """of_warp_bwd_det_cv's dflow_add (the FlowAdd path) in every kernel that forms d(flow):
    the tile kernel, the scalar kernel and the window kernel above key 28."""
    _, _, _, _, dinp_ref, dflow_ref = case(si, family)
    n, h, w, c = SHAPES[si]
    add = rng_tensor((n, h, w, 4), 91 + si)
    dinp, dflow, _, _ = det_call(si, family, dev(add))
    assert rel_inf(dinp, dinp_ref) < REL_TOL
    assert rel_inf(dflow, dflow_ref + f64(add)[..., :2]) < REL_TOL
    plain = det_call(si, family)
    assert torch.equal(dinp, plain[0])


# ------------------------------------------- 4. _cv(..., 0) is the old entry point -----
def _photo_inputs(levels, n, seed):
    imgs = [dev(rng_tensor((n, h, w, 6), seed + i, lo=-0.5, hi=0.6))
            for i, (h, w) in enumerate(levels)]
    flows = [dev(_off_integer(rng_tensor((n, h, w, 2), seed + 50 + i, scale=2.0)))
             for i, (h, w) in enumerate(levels)]
    return imgs, flows


def _photo_fwd(name, imgs, flows, n, levels, *cv):
    from optical_flow_amd._lib import call
    nparts = [_lib().of_photo_l1_partials(n, h, w) for h, w in levels]
    parts = torch.full((sum(nparts),), float("nan"), device="cuda")
    call(name, _ptrs(imgs), _ptrs(flows), n, _arr(C.c_int, [h for h, _ in levels]),
         _arr(C.c_int, [w for _, w in levels]), len(levels), P(parts), *cv, None)
    torch.cuda.synchronize()
    return parts, nparts


def _photo_bwd(name, imgs, flows, n, levels, coefs, ld, *cv):
    from optical_flow_amd._lib import call
    outs = [torch.full((n, h, w, ld), -3.0, device="cuda") for h, w in levels]
    call(name, _ptrs(imgs), _ptrs(flows), n, _arr(C.c_int, [h for h, _ in levels]),
         _arr(C.c_int, [w for _, w in levels]), len(levels), _arr(C.c_float, coefs), None,
         _ptrs(outs), _arr(C.c_int, [ld] * len(levels)), *cv, None)
    torch.cuda.synchronize()
    return outs


def _census_fwd(name, imgs, flows, n, levels, r, coefs, *cv):
    from optical_flow_amd._lib import call
    nparts = [_lib().of_census_partials(n, h, w) for h, w in levels]
    parts = torch.full((sum(nparts),), float("nan"), device="cuda")
    planes = [torch.full((n, h, w, 2), float("nan"), device="cuda") for h, w in levels]
    call(name, _ptrs(imgs), _ptrs(flows), n, _arr(C.c_int, [h for h, _ in levels]),
         _arr(C.c_int, [w for _, w in levels]), len(levels), r, _arr(C.c_float, coefs), None,
         _ptrs(planes), P(parts), *cv, None)
    torch.cuda.synchronize()
    return parts, nparts, planes


def test_cv_reference_is_the_old_entry_point():
    """Every _cv entry point with convention 0 bitwise equal to the entry point without the
    suffix.  The atomic backward's d(features) is a sum whose order the hardware picks (LDS
    ranks, float atomics), so two calls of the SAME entry point differ in the last bit on a
    random flow; it is compared bitwise on a flow for which the sum has no order -- the
    integer flow (j - i, i - j), which in the reference convention samples every pixel at
    itself with weights exactly 1, 0, 0, 0, one non-zero term per destination -- and on the
    random flow d(flow), which is formed in a fixed order, is compared bitwise and
    d(features) to the atomic form's own run-to-run noise (1e-6)."""
    from optical_flow_amd._lib import call
    lib = _lib()
    shape = (2, 6, 8, 64)
    n, h, w, c = shape
    inp, flow, g = dev(rng_tensor(shape, 5)), dev(rng_tensor((n, h, w, 2), 6, scale=1.5)), \
        dev(rng_tensor(shape, 7))
    add = dev(rng_tensor((n, h, w, 4), 8))
    o0, o1 = torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda")
    call("of_warp_fwd", P(inp), n, h, w, c, P(flow), P(o0), None)
    call("of_warp_fwd_cv", P(inp), n, h, w, c, P(flow), P(o1), 0, None)
    assert torch.equal(o0, o1)
    res = []
    for cv in (False, True):
        for with_add in (False, True):
            dinp = torch.zeros(shape, device="cuda")
            dfl = torch.empty((n, h, w, 2), device="cuda")
            if cv:
                call("of_warp_bwd_cv", P(g), P(inp), n, h, w, c, P(flow), P(dinp), P(dfl),
                     P(add) if with_add else None, 4 if with_add else 0, 0, None)
            elif with_add:
                call("of_warp_bwd_add", P(g), P(inp), n, h, w, c, P(flow), P(dinp), P(dfl),
                     P(add), 4, None)
            else:
                call("of_warp_bwd", P(g), P(inp), n, h, w, c, P(flow), P(dinp), P(dfl), None)
            res.append((dinp, dfl))
    torch.cuda.synchronize()
    for k in (0, 1):
        assert rel_inf(res[k][0], res[2 + k][0]) < 1e-6
        assert torch.equal(res[k][1], res[2 + k][1])
    ii, jj = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
    perm = dev(torch.stack([jj - ii, ii - jj], -1).expand(n, h, w, 2).contiguous())
    res = []
    for cv in (False, True):
        dinp = torch.zeros(shape, device="cuda")
        dfl = torch.empty((n, h, w, 2), device="cuda")
        if cv:
            call("of_warp_bwd_cv", P(g), P(inp), n, h, w, c, P(perm), P(dinp), P(dfl), None, 0,
                 0, None)
        else:
            call("of_warp_bwd", P(g), P(inp), n, h, w, c, P(perm), P(dinp), P(dfl), None)
        res.append((dinp, dfl))
    torch.cuda.synchronize()
    assert torch.equal(res[0][0], g)                      # (the identity's adjoint)
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    wsb = lib.of_warp_bwd_det_workspace(n, h, w, c)
    det = []
    for cv in (False, True):
        ws = torch.zeros((wsb + 3) // 4, dtype=torch.int32, device="cuda")
        dinp = torch.empty(shape, device="cuda")
        dfl = torch.empty((n, h, w, 2), device="cuda")
        if cv:
            call("of_warp_bwd_det_cv", P(g), P(inp), n, h, w, c, P(flow), P(dinp), P(dfl),
                 P(add), 4, 0, P(ws), wsb, None)
        else:
            call("of_warp_bwd_det", P(g), P(inp), n, h, w, c, P(flow), 0, P(dinp), P(dfl),
                 P(add), 4, P(ws), wsb, None)
        det.append((dinp, dfl))
    torch.cuda.synchronize()
    assert torch.equal(det[0][0], det[1][0]) and torch.equal(det[0][1], det[1][1])
    levels = [(5, 7), (9, 6)]
    imgs, flows = _photo_inputs(levels, n, 20)
    p0, _ = _photo_fwd("of_photo_l1_fwd_multi", imgs, flows, n, levels)
    p1, _ = _photo_fwd("of_photo_l1_fwd_multi_cv", imgs, flows, n, levels, 0)
    assert torch.equal(p0, p1)
    b0 = _photo_bwd("of_photo_l1_bwd_multi", imgs, flows, n, levels, [0.5, 2.0], 4)
    b1 = _photo_bwd("of_photo_l1_bwd_multi_cv", imgs, flows, n, levels, [0.5, 2.0], 4, 0)
    assert all(torch.equal(x, y) for x, y in zip(b0, b1))
    c0 = _census_fwd("of_census_fwd_multi", imgs, flows, n, levels, 3, [1.0, 1.0])
    c1 = _census_fwd("of_census_fwd_multi_cv", imgs, flows, n, levels, 3, [1.0, 1.0], 0)
    assert torch.equal(c0[0], c1[0])
    assert all(torch.equal(x, y) for x, y in zip(c0[2], c1[2]))


# ---------------------------------------------------------------- 5. loss kernels ------
LEVELS = [(5, 7), (9, 6)]                    # odd level sizes, both in one call


def test_photo_kernels_image_convention():
    """of_photo_l1_fwd_multi_cv / _bwd_multi_cv in the image convention, two odd-sized levels
    in one call, d(flow) into padded rows (ld 4, the pad untouched), against the patched
    reference's per-level sums and float64 autograd."""
    n = 2
    imgs, flows = _photo_inputs(LEVELS, n, 30)
    parts, nparts = _photo_fwd("of_photo_l1_fwd_multi_cv", imgs, flows, n, LEVELS, IMAGE)
    coefs = [0.5, 2.0]
    outs = _photo_bwd("of_photo_l1_bwd_multi_cv", imgs, flows, n, LEVELS, coefs, 4, IMAGE)
    o = 0
    with image_convention():
        for l, (im, f) in enumerate(zip(imgs, flows)):
            fo = f64(f).requires_grad_(True)
            i6 = f64(im)
            s = (i6[..., :3] - R.warp_features(fo, i6[..., 3:])).abs().sum()
            got = parts[o:o + nparts[l]].double().sum().item()
            o += nparts[l]
            assert abs(got - s.item()) / s.item() < REL_TOL, (l, got, s.item())
            gref = torch.autograd.grad(coefs[l] * s, fo)[0]
            assert rel_l2(outs[l][..., :2], gref) < REL_TOL, l
            assert (outs[l][..., 2:] == -3.0).all()


@pytest.mark.parametrize("r", [1, 3])
def test_census_kernels_image_convention(r):
    """of_census_fwd_multi_cv in the image convention (radius 1 and 3), the same two levels:
    C_l and d C_l / d flow against tests/census_ref.py under the patched warp; the backward's
    padded rows."""
    from optical_flow_amd._lib import call
    n = 2
    imgs, flows = _photo_inputs(LEVELS, n, 40)
    coefs = [0.25, 1.5]
    parts, nparts, planes = _census_fwd("of_census_fwd_multi_cv", imgs, flows, n, LEVELS, r,
                                        coefs, IMAGE)
    outs = [torch.full((n, h, w, 4), -3.0, device="cuda") for h, w in LEVELS]
    call("of_census_bwd_multi", _ptrs(planes), n, _arr(C.c_int, [h for h, _ in LEVELS]),
         _arr(C.c_int, [w for _, w in LEVELS]), len(LEVELS), _arr(C.c_float, coefs), None,
         _ptrs(outs), _arr(C.c_int, [4] * len(LEVELS)), 0, None)
    torch.cuda.synchronize()
    o = 0
    with image_convention():
        for l, (im, f) in enumerate(zip(imgs, flows)):
            fo = f64(f).requires_grad_(True)
            cl = census_ref.level_sum(*census_ref.gray_pair(f64(im), fo), r)
            got = parts[o:o + nparts[l]].double().sum().item()
            o += nparts[l]
            assert abs(got - coefs[l] * cl.item()) / (coefs[l] * cl.item()) < REL_TOL, (l, got)
            gref = torch.autograd.grad(cl, fo)[0]
            assert rel_l2(planes[l], gref) < REL_TOL, l
            assert rel_l2(outs[l][..., :2], coefs[l] * gref) < REL_TOL, l
            assert (outs[l][..., 2:] == -3.0).all()


def test_known_answer_on_the_device():
    """The point of the convention, on the device: a pair shifted by (dx, dy) = (16, -16) with
    the true flow (-dx, -dy) / 2^(s+1) at four scales.  The pair is cropped so that every
    pixel is interior: the content sits in a flat frame wider than the shift plus the resize
    support at every level, so no sample of any pixel reaches a value that edge replication
    made up.  Per level, the photometric partials' sum is <= 1e-6 times the zero-flow sum of
    the same images (and is not in the reference convention); the census term likewise."""
    ops = _ops()
    Hh, Ww, dx, dy, frame = 128, 160, 16, -16, 40
    pair = shifted_pair(Hh, Ww, 0, 0, seed=3, dtype=torch.float32)[..., :3]
    flat = torch.full_like(pair, 0.5)
    flat[:, frame:Hh - frame, frame:Ww - frame] = pair[:, frame:Hh - frame, frame:Ww - frame]
    ys = (torch.arange(Hh) + dy).clamp(0, Hh - 1)
    xs = (torch.arange(Ww) + dx).clamp(0, Ww - 1)
    batch = dev(torch.cat([flat, flat[:, ys][:, :, xs]], -1))
    levels = [(Hh >> (s + 1), Ww >> (s + 1)) for s in range(4)]
    true = [torch.tensor([-dx / 2.0 ** (s + 1), -dy / 2.0 ** (s + 1)], device="cuda")
            .expand(1, h, w, 2).contiguous() for s, (h, w) in enumerate(levels)]
    zero = [torch.zeros_like(f) for f in true]
    pyr = ops._pyramid6(batch, true)
    sums = {}
    for name, fl, cv in (("true", true, IMAGE), ("zero", zero, IMAGE), ("ref", true, 0)):
        parts, nparts = _photo_fwd("of_photo_l1_fwd_multi_cv", pyr, fl, 1, levels, cv)
        o, sums[name] = 0, []
        for k in nparts:
            sums[name].append(parts[o:o + k].double().sum().item())
            o += k
    print("photometric sums per level:", sums)
    for l in range(4):
        assert sums["zero"][l] > 1.0
        assert sums["true"][l] <= 1e-6 * sums["zero"][l], (l, sums)
        assert sums["ref"][l] > 0.1 * sums["zero"][l], (l, sums)
    c_true = ops.census_loss(batch, true, 3, convention="image").item()
    c_zero = ops.census_loss(batch, zero, 3, convention="image").item()
    print("census:", c_true, c_zero)
    assert c_zero > 1e-3 and c_true <= 1e-6 * c_zero


# ------------------------------------------------------------------ 6. whole step ------
def _setup(H, W, B, seed=0, **kw):
    """As tests/test_gpu_model.py::_setup builds its inputs."""
    from optical_flow_amd.data import synthetic_batch
    from optical_flow_amd.model import FlowNet
    from optical_flow_amd.params import encoder_blocks, flow_net_spec, init_params, perturb_params
    vals = perturb_params(init_params(flow_net_spec(), seed), seed + 1)
    net = FlowNet(H, W, values=vals, **kw)
    batch = synthetic_batch(B, H, W, seed=1234 + seed)
    return net, vals, batch, list(encoder_blocks())


def _sign_report(batch, flows_dev, flows_ref):
    """The pixels whose photometric residual changes sign between the device flows and the
    oracle's (the |.| kink: a gradient there is not comparable at 1e-3)."""
    b = torch.tensor(batch, dtype=torch.float64)
    H, W = b.shape[1], b.shape[2]
    with image_convention():
        for s, (fd, fr) in enumerate(zip(flows_dev, flows_ref)):
            h, w = H >> (s + 1), W >> (s + 1)
            r = R.resize_bilinear(b, h, w)
            d0 = r[..., :3] - R.warp_features(f64(fr), r[..., 3:])
            d1 = r[..., :3] - R.warp_features(f64(fd), r[..., 3:])
            idx = (torch.sign(d0) != torch.sign(d1)).nonzero()
            print("scale %d: %d residual signs differ" % (s, len(idx)))
            for t in idx[:8].tolist():
                print("  ", t, d0[tuple(t)].item(), d1[tuple(t)].item())


@pytest.mark.parametrize("seed", [0, 1])
def test_whole_step_image_convention(seed):
    """FlowNet(64, 128, warp_convention="image"), B = 2, against the patched float64 oracle's
    train_step: loss, the four flows and every gradient."""
    from optical_flow_amd.loss import LossLayer
    net, vals, batch, blocks = _setup(64, 128, 2, seed, warp_convention="image")
    assert net.warp_convention == "image"
    p = {k: torch.tensor(v, dtype=torch.float64) for k, v in vals.items()}
    with image_convention():
        loss_o, flows_o, grads_o = R.train_step(torch.tensor(batch, dtype=torch.float64), p,
                                                blocks, None)
    net.store.zero_grad()
    bd = dev(torch.from_numpy(batch))
    flows = net(bd)
    loss = LossLayer(warp_convention="image")(bd, flows)
    loss.backward()
    torch.cuda.synchronize()
    errs = sorted(((rel_l2(g, grads_o[k]), k) for k, g in net.store.grads().items()),
                  reverse=True)
    ferr = [rel_inf(f, fo) for f, fo in zip(flows, flows_o)]
    lerr = abs(loss.item() - loss_o.item()) / abs(loss_o.item())
    print("seed %d: loss rel %.2e, flows %s, worst gradients %s" % (seed, lerr, ferr, errs[:3]))
    if max(ferr) >= REL_TOL or lerr >= REL_TOL or errs[0][0] >= REL_TOL:
        _sign_report(batch, flows, flows_o)
    assert max(ferr) < REL_TOL
    assert lerr < REL_TOL
    assert errs[0][0] < REL_TOL, errs[0]


def test_whole_step_image_convention_all_terms():
    """Seed 0 with the census term (radius 3), smoothness 0.2 and edge alpha 10 on: loss =
    photometric + census (tests/census_ref.py under the patch) + 0.2 smoothness."""
    from optical_flow_amd.loss import LossLayer
    from optical_flow_amd.train import Trainer
    net, vals, batch, blocks = _setup(64, 128, 2, 0, warp_convention="image")
    p = {k: torch.tensor(v, dtype=torch.float64) for k, v in vals.items()}
    tr = {k: v.requires_grad_(True) for k, v in p.items()
          if not k.endswith(("moving_mean", "moving_variance"))}
    b = torch.tensor(batch, dtype=torch.float64)
    with image_convention():
        flows_o = R.flow_net(b, p, blocks)
        loss_o = (R.photometric_loss(b, flows_o) + census_ref.census(b, flows_o, 3) +
                  0.2 * ref_smooth(b, flows_o, 10.0))
        loss_o.backward()
    layer = LossLayer(0.2, 10.0, census_weight=1.0, census_radius=3, warp_convention="image")
    trainer = Trainer(net, loss_layer=layer)
    net.store.zero_grad()
    bd = dev(torch.from_numpy(batch))
    flows = net(bd)
    loss = layer(bd, flows)
    loss.backward()
    torch.cuda.synchronize()
    errs = sorted(((rel_l2(g, tr[k].grad), k) for k, g in net.store.grads().items()),
                  reverse=True)
    lerr = abs(loss.item() - loss_o.item()) / abs(loss_o.item())
    print("loss rel %.2e, worst gradients %s" % (lerr, errs[:3]))
    assert lerr < REL_TOL
    assert errs[0][0] < REL_TOL, errs[0]
    assert trainer.loss_layer is layer


# ----------------------------------------------------------- 7. default unchanged ------
def test_default_is_the_reference_convention():
    """FlowNet(64, 128) and FlowNet(64, 128, warp_convention="reference"): bitwise equal
    flows, loss and gradients (and not the image convention's)."""
    from optical_flow_amd.loss import LossLayer
    res = []
    for kw, lkw in (({}, {}), (dict(warp_convention="reference"),
                               dict(warp_convention="reference")),
                    (dict(warp_convention="image"), dict(warp_convention="image"))):
        net, _, batch, _ = _setup(64, 128, 2, 0, **kw)
        net.store.zero_grad()
        bd = dev(torch.from_numpy(batch))
        flows = net(bd)
        loss = LossLayer(**lkw)(bd, flows)
        loss.backward()
        torch.cuda.synchronize()
        res.append((loss.detach().clone(), [f.detach().clone() for f in flows],
                    {k: g.detach().clone() for k, g in net.store.grads().items()}))
    assert res[0][0].item() == res[1][0].item()
    assert all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1]))
    assert all(torch.equal(g, res[1][2][k]) for k, g in res[0][2].items())
    assert not torch.equal(res[0][1][0], res[2][1][0])
