"""Occlusion masks and the data terms that honour them (DESIGN.md "Occlusion masks";
include/oflow.h of_occ_mask_multi, of_photo_l1_*_multi_w, of_census_fwd_multi_w): the kernels
through the C ABI, known answers, ops.occlusion_masks, LossLayer(occlusion=...), and a whole
forward-backward train step, eager and captured, against the float64 restatement of the
definitions in tests/occlusion_ref.py.  Tolerance: the project's REL_TOL (rel_l2 on gradients,
relative error on scalars).  The masks are compared exactly, on every pixel whose decision is
not within rounding of its threshold (tests/test_occlusion_host.py bounds how many those are
and shows the loss-parity inputs have none)."""
import ctypes as C
import functools

import pytest
import torch

import occlusion_ref as O
from helpers import REL_TOL, dev, f64, rel_l2, rng_tensor
from test_gpu_census import CASES, N
from test_gpu_smooth_loss import ref_smooth
from warp_image_ref import shifted_pair, true_flows

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _rel(a, b):
    return abs(a - b) / abs(b)


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def _ptrs(ts):
    """A pointer array; a None entry is a NULL pointer."""
    return _arr(C.c_void_p, [t.data_ptr() if t is not None else None for t in ts])


def _hw(levels):
    return _arr(C.c_int, [h for h, _ in levels]), _arr(C.c_int, [w for _, w in levels])


# ------------------------------------------------------------------------ 1. mask kernel ----
def _mask_status(flows, n, stride, levels, mode, alpha1, alpha2s, masks=None, nlevels=None,
                 null_flows=False, null_masks=False):
    """of_occ_mask_multi's status and the NaN-prefilled outputs."""
    from optical_flow_amd import _lib, ops
    if masks is None:
        masks = [torch.full((max(n, 1), h, w), NAN, device="cuda") for h, w in levels]
    hs, ws = _hw(levels)
    st = _lib.lib().of_occ_mask_multi(
        None if null_flows else _ptrs(flows), n, stride, hs, ws,
        len(levels) if nlevels is None else nlevels, mode, alpha1,
        _arr(C.c_float, alpha2s) if alpha2s is not None else None,
        None if null_masks else _ptrs(masks), ops._stream())
    torch.cuda.synchronize()
    return st, masks


def _masks(flows, mode, alpha2s=None, alpha1=O.ABI_ALPHA1):
    from optical_flow_amd import _lib
    n = flows[0].shape[0]
    levels = [(f.shape[1], f.shape[2]) for f in flows]
    code = {"border": _lib.OCC_BORDER, "fb": _lib.OCC_FB}[mode]
    st, masks = _mask_status(flows, n, n // 2, levels, code, alpha1,
                             alpha2s if alpha2s is not None else [0.0] * len(levels))
    assert st == 0, _lib.lib().of_last_error()
    return masks


@pytest.mark.parametrize("mode", ["border", "fb"])
def test_mask_kernel_abi(mode):
    """Four levels (1 x 1, under a block, ragged, several blocks) in one launch, n = 4: every
    element written (NaN prefill), exactly 0.0 or 1.0, equal to the reference on every pixel
    that is not near a decision; in fb mode exchanging the two pairs' backward flows changes
    the masks (the partner of image b is b + B, not some other image)."""
    flows = O.abi_flows(mode)
    fd = [dev(f) for f in flows]
    got = _masks(fd, mode, O.ABI_ALPHA2S)
    for l, (f, m) in enumerate(zip(flows, got)):
        a2 = O.ABI_ALPHA2S[l]
        want = O.border(f64(f))[0] if mode == "border" else O.fb(f64(f), O.ABI_ALPHA1, a2)[0]
        nr = O.near(f64(f), mode, O.ABI_ALPHA1, a2)
        m = m.cpu()
        assert ((m == 0.0) | (m == 1.0)).all()
        differ = (m.double() != want) & ~nr
        print(mode, tuple(f.shape), "valid", m.mean().item(), "near", int(nr.sum()),
              "differ", int(differ.sum()))
        assert not differ.any()
    if mode == "fb":
        B = O.ABI_N // 2
        swapped = [torch.cat([f[:B], f[B:].flip(0)], 0).contiguous() for f in fd]
        other = _masks(swapped, mode, O.ABI_ALPHA2S)
        for l in (2, 3):
            assert not torch.equal(other[l][:B], got[l][:B])


def test_mask_known_answers():
    """Zero flows: all ones in both modes.  Forward (+2, 0) with backward (-2, 0): consistent
    wherever the sample is in the frame, so the forward mask is 0 in exactly the last two
    columns and the backward mask in exactly the first two.  The backward flow off by 3 px
    inside a rectangle: 0 where the forward samples land in it."""
    h, w, B = 13, 21, 2
    z = torch.zeros(2 * B, h, w, 2, device="cuda")
    for mode in ("border", "fb"):
        assert (_masks([z], mode, [0.5])[0] == 1.0).all()
    f = z.clone()
    f[:B, ..., 0], f[B:, ..., 0] = 2.0, -2.0
    m = _masks([f], "fb", [0.5])[0]
    want = torch.ones(2 * B, h, w, device="cuda")
    want[:B, :, w - 2:] = 0.0
    want[B:, :, :2] = 0.0
    assert torch.equal(m, want)
    assert torch.equal(_masks([f], "border")[0], want)
    g = f.clone()
    g[B:, 4:9, 6:12, 0] += 3.0                  # rows 4..8, columns 6..11 of the backward flows
    m = _masks([g], "fb", [0.5])[0]
    want[:B, 4:9, 4:10] = 0.0                   # the forward pixels whose sample (j + 2) is there
    # the backward pixels of the rectangle now sample (j + 1, i): in the frame, where the
    # forward flow is +2: |1 + 2|^2 > threshold
    want[B:, 4:9, 6:12] = 0.0
    assert torch.equal(m, want)


def test_mask_border_is_inclusive():
    """A sample exactly on x = w - 1 or on y = 0 is valid; one ulp-scale step beyond is not."""
    h, w = 5, 8
    f = torch.zeros(1, h, w, 2)
    f[0, :, :, 0] = (w - 1) - torch.arange(w, dtype=torch.float32)      # every x = w - 1
    f[0, :, :, 1] = -torch.arange(h, dtype=torch.float32)[:, None]      # every y = 0
    assert (_masks([dev(f)], "border")[0] == 1.0).all()
    g = f.clone()
    g[0, 2, 3, 0] += 0.001
    g[0, 4, 1, 1] -= 0.001
    m = _masks([dev(g)], "border")[0].cpu()
    want = torch.ones(1, h, w)
    want[0, 2, 3] = want[0, 4, 1] = 0.0
    assert torch.equal(m, want)


def test_mask_einval_launches_nothing():
    from optical_flow_amd import _lib
    levels = [(5, 3), (13, 21)]
    flows = [torch.zeros(4, h, w, 2, device="cuda") for h, w in levels]
    BORDER, FB = _lib.OCC_BORDER, _lib.OCC_FB
    ok = dict(flows=flows, n=4, stride=2, levels=levels, mode=FB, alpha1=0.01, alpha2s=[0.5, 0.5])
    bad = [dict(nlevels=0), dict(nlevels=9), dict(n=0, stride=0), dict(mode=0), dict(mode=3),
           dict(stride=1), dict(stride=4), dict(n=3, stride=1), dict(stride=0, n=0),
           dict(alpha1=-0.01), dict(mode=BORDER, alpha1=-0.01), dict(alpha2s=None),
           dict(alpha2s=[0.5, -0.5]), dict(levels=[(5, 3), (0, 21)]),
           dict(levels=[(5, 0), (13, 21)]), dict(null_flows=True), dict(null_masks=True),
           dict(mode=BORDER, null_masks=True)]
    for kw in bad:
        outs = [torch.full((4, 5, 3), NAN, device="cuda"), torch.full((4, 13, 21), NAN, device="cuda")]
        st, _ = _mask_status(**{**ok, **kw, "masks": outs})
        assert st == _lib.OF_EINVAL, kw
        assert all(torch.isnan(o).all() for o in outs), kw
    st, outs = _mask_status(**ok)
    assert st == 0 and all((o == 1.0).all() for o in outs)
    # border mode reads neither the stride nor alpha2s, and takes an odd n
    st, outs = _mask_status(**{**ok, "mode": BORDER, "n": 3, "stride": 0, "alpha2s": None,
                               "flows": [f[:3].contiguous() for f in flows]})
    assert st == 0 and all((o == 1.0).all() for o in outs)


# ------------------------------------------------------ 2. weighted photometric kernels ----
def _weights(levels, seed):
    return [rng_tensor((N, h, w), seed + i, lo=0.0, hi=1.0) for i, (h, w) in enumerate(levels)]


@functools.lru_cache(maxsize=None)
def _case(idx):
    """CASES[idx]'s levels and radius (tests/test_gpu_census.py) with flows of scale 3, images
    and weights in [0, 1]; per level the float64 references in the image convention: weighted
    photometric sum and its d(flow), weighted C_l and its d(flow)."""
    levels, r = CASES[idx]
    flows = [rng_tensor((N, h, w, 2), 300 + i, scale=3.0) for i, (h, w) in enumerate(levels)]
    imgs = [rng_tensor((N, h, w, 6), 400 + i, lo=-0.5, hi=0.6) for i, (h, w) in enumerate(levels)]
    wts = _weights(levels, 500)
    ref = []
    for f, im, wt in zip(flows, imgs, wts):
        fo = f64(f).requires_grad_(True)
        p = O.photo_level(f64(im), fo, f64(wt))
        c = O.census_level(*O.gray_pair(f64(im), fo), f64(wt), r)
        gp = torch.autograd.grad(p, fo)[0] if p.requires_grad else torch.zeros_like(fo)
        gc = torch.autograd.grad(c, fo)[0] if c.requires_grad else torch.zeros_like(fo)
        ref.append((p.item(), gp, c.item(), gc))
    return levels, r, flows, imgs, wts, ref


def _level_sums(parts, nparts):
    sums, o = [], 0
    for k in nparts:
        sums.append(parts[o:o + k].double().sum().item())
        o += k
    return sums


def _photo_fwd(imgs, flows, wts, levels):
    """of_photo_l1_fwd_multi_w (wts: a list with None entries, or None for a NULL array), or
    of_photo_l1_fwd_multi_cv when wts == "cv"; image convention.  (level sums, partials)"""
    from optical_flow_amd import _lib, ops
    from optical_flow_amd._lib import call
    nparts = [_lib.lib().of_photo_l1_partials(N, h, w) for h, w in levels]
    parts = torch.full((sum(nparts),), NAN, device="cuda")
    hs, ws = _hw(levels)
    if isinstance(wts, str):
        call("of_photo_l1_fwd_multi_cv", _ptrs(imgs), _ptrs(flows), N, hs, ws, len(levels),
             ops._ptr(parts), _lib.WARP_IMAGE, ops._stream())
    else:
        call("of_photo_l1_fwd_multi_w", _ptrs(imgs), _ptrs(flows),
             _ptrs(wts) if wts is not None else None, N, hs, ws, len(levels), ops._ptr(parts),
             _lib.WARP_IMAGE, ops._stream())
    torch.cuda.synchronize()
    return _level_sums(parts, nparts), parts


def _photo_bwd(imgs, flows, wts, levels, coefs, dloss, ld, fill):
    from optical_flow_amd import _lib, ops
    from optical_flow_amd._lib import call
    outs = [torch.full((N, h, w, ld), fill, device="cuda") for h, w in levels]
    hs, ws = _hw(levels)
    L = len(levels)
    if isinstance(wts, str):
        call("of_photo_l1_bwd_multi_cv", _ptrs(imgs), _ptrs(flows), N, hs, ws, L,
             _arr(C.c_float, coefs), ops._ptr(dloss), _ptrs(outs), _arr(C.c_int, [ld] * L),
             _lib.WARP_IMAGE, ops._stream())
    else:
        call("of_photo_l1_bwd_multi_w", _ptrs(imgs), _ptrs(flows),
             _ptrs(wts) if wts is not None else None, N, hs, ws, L, _arr(C.c_float, coefs),
             ops._ptr(dloss), _ptrs(outs), _arr(C.c_int, [ld] * L), _lib.WARP_IMAGE,
             ops._stream())
    torch.cuda.synchronize()
    return outs


def _null_entry(ones):
    """Weights of ones with a NULL entry (two where there are levels enough: the first and
    the last level)."""
    out = list(ones)
    out[0] = None
    if len(out) > 2:
        out[-1] = None
    return out


@pytest.mark.parametrize("idx", [0, 1, 2], ids=lambda i: "case%d" % i)
def test_weighted_photometric_kernels(idx):
    """Per level the partial slice sums to sum_p w[p] sum_c |diff| and d(flow) is coefs[l] * g
    * its gradient, at stride 2 and at stride 4 with the padding untouched.  Weights of ones,
    a NULL array and a NULL entry are bitwise the `_cv` entry points; weights of zeros give
    exactly 0."""
    levels, _, flows, imgs, wts, ref = _case(idx)
    L = len(levels)
    fd, idv, wd = [dev(f) for f in flows], [dev(i) for i in imgs], [dev(w) for w in wts]
    coefs = [0.3 + 0.1 * l for l in range(L)]
    g = 1.75
    dloss = torch.tensor([g], device="cuda")
    sums, _ = _photo_fwd(idv, fd, wd, levels)
    d2 = _photo_bwd(idv, fd, wd, levels, coefs, dloss, 2, NAN)
    d4 = _photo_bwd(idv, fd, wd, levels, coefs, dloss, 4, 7.0)
    for l, (h, w) in enumerate(levels):
        want, grad = ref[l][0], ref[l][1] * (coefs[l] * g)
        e2, e4 = rel_l2(d2[l], grad), rel_l2(d4[l][..., :2], grad)
        print("level", (h, w), "value", sums[l], want, "d(flow) rel_l2 ld2 %.2e ld4 %.2e" % (e2, e4))
        assert _rel(sums[l], want) < REL_TOL
        if (h, w) == (1, 1):
            # all four corners are the one pixel: the gradient is 0 (autograd leaves the
            # rounding of b*v + (1-b)*v - b*v - (1-b)*v, no scale to compare against)
            assert grad.abs().max().item() < 1e-12 and (d2[l] == 0).all()
        else:
            assert e2 < REL_TOL and e4 < REL_TOL
        assert torch.equal(d2[l], d4[l][..., :2]) and (d4[l][..., 2:] == 7.0).all()
    # weight 1 in its three spellings: bitwise the unweighted entry points
    ones = [torch.ones(N, h, w, device="cuda") for h, w in levels]
    _, parts_cv = _photo_fwd(idv, fd, "cv", levels)
    grads_cv = _photo_bwd(idv, fd, "cv", levels, coefs, dloss, 4, 7.0)
    for spelling in (ones, None, _null_entry(ones)):
        _, parts = _photo_fwd(idv, fd, spelling, levels)
        assert torch.equal(parts, parts_cv)
        for a, b in zip(_photo_bwd(idv, fd, spelling, levels, coefs, dloss, 4, 7.0), grads_cv):
            assert torch.equal(a, b)
    zeros = [torch.zeros(N, h, w, device="cuda") for h, w in levels]
    _, parts = _photo_fwd(idv, fd, zeros, levels)
    assert (parts == 0).all()
    for d in _photo_bwd(idv, fd, zeros, levels, coefs, dloss, 2, NAN):
        assert (d == 0).all()


# ------------------------------------------------------------- 3. weighted census forward ----
def _census_fwd(imgs, flows, wts, levels, r, coefs):
    """of_census_fwd_multi_w (wts as in _photo_fwd), or of_census_fwd_multi_cv for "cv"; image
    convention.  (level sums, partials, planes)"""
    from optical_flow_amd import _lib, ops
    from optical_flow_amd._lib import call
    nparts = [_lib.lib().of_census_partials(N, h, w) for h, w in levels]
    parts = torch.full((sum(nparts),), NAN, device="cuda")
    planes = [torch.full((N, h, w, 2), NAN, device="cuda") for h, w in levels]
    hs, ws = _hw(levels)
    if isinstance(wts, str):
        call("of_census_fwd_multi_cv", _ptrs(imgs), _ptrs(flows), N, hs, ws, len(levels), r,
             _arr(C.c_float, coefs), None, _ptrs(planes), ops._ptr(parts), _lib.WARP_IMAGE,
             ops._stream())
    else:
        call("of_census_fwd_multi_w", _ptrs(imgs), _ptrs(flows),
             _ptrs(wts) if wts is not None else None, N, hs, ws, len(levels), r,
             _arr(C.c_float, coefs), None, _ptrs(planes), ops._ptr(parts), _lib.WARP_IMAGE,
             ops._stream())
    torch.cuda.synchronize()
    return _level_sums(parts, nparts), parts, planes


@pytest.mark.parametrize("idx", [0, 1, 2], ids=lambda i: "case%d_r%d" % (i, CASES[i][1]))
def test_weighted_census_forward(idx):
    """Per level the partial slice sums to coefs[l] * C_l with the centre weights and the plane
    is autograd's d C_l / d flow of that definition.  Ones, a NULL array and a NULL entry are
    bitwise of_census_fwd_multi_cv (partials and planes); zeros give exactly 0."""
    levels, r, flows, imgs, wts, ref = _case(idx)
    L = len(levels)
    fd, idv, wd = [dev(f) for f in flows], [dev(i) for i in imgs], [dev(w) for w in wts]
    coefs = [0.3 + 0.1 * l for l in range(L)]
    sums, _, planes = _census_fwd(idv, fd, wd, levels, r, coefs)
    for l, (h, w) in enumerate(levels):
        want = coefs[l] * ref[l][2]
        ep = rel_l2(planes[l], ref[l][3])
        print("level", (h, w), "r", r, "value", sums[l], want, "plane rel_l2 %.2e" % ep)
        if (h, w) == (1, 1):
            assert sums[l] == 0.0 and want == 0.0 and (planes[l] == 0).all()
        else:
            assert _rel(sums[l], want) < REL_TOL
        assert ep < REL_TOL
    ones = [torch.ones(N, h, w, device="cuda") for h, w in levels]
    _, parts_cv, planes_cv = _census_fwd(idv, fd, "cv", levels, r, coefs)
    for spelling in (ones, None, _null_entry(ones)):
        _, parts, pl = _census_fwd(idv, fd, spelling, levels, r, coefs)
        assert torch.equal(parts, parts_cv)
        for a, b in zip(pl, planes_cv):
            assert torch.equal(a, b)
    zeros = [torch.zeros(N, h, w, device="cuda") for h, w in levels]
    _, parts, pl = _census_fwd(idv, fd, zeros, levels, r, coefs)
    assert (parts == 0).all() and all((p == 0).all() for p in pl)


@pytest.mark.parametrize("r", [1, 3])
def test_census_weight_reach_and_halo(r):
    """On the 40 x 57 level (five tile rows, two tile columns): a weight plane that is 1 at one
    interior pixel gives a plane that is exactly 0 farther than r from it (and in the other
    image) and non-zero at it; two weight planes that differ in one pixel of a tile's halo --
    the row above the tile, then the column right of it -- change that tile's plane (the halo
    weights are loaded, not taken as 1 or 0)."""
    levels, _, flows, imgs, wts, _ = _case(1)
    h, w = levels[1]
    assert (h, w) == (40, 57)
    f, im = [dev(flows[1])], [dev(imgs[1])]
    y0, x0 = 20, 30
    one = torch.zeros(N, h, w, device="cuda")
    one[0, y0, x0] = 1.0
    sums, _, (pl,) = _census_fwd(im, f, [one], [(h, w)], r, [1.0])
    far = torch.ones(N, h, w, dtype=torch.bool, device="cuda")
    far[0, y0 - r:y0 + r + 1, x0 - r:x0 + r + 1] = False
    assert (pl[far] == 0).all() and sums[0] > 0
    assert (pl[0, y0, x0] != 0).any()
    assert (pl[0, y0 - r:y0 + r + 1, x0 - r:x0 + r + 1] != 0).sum() > 2
    base = dev(wts[1])
    _, _, (pa,) = _census_fwd(im, f, [base], [(h, w)], r, [1.0])
    tile = (0, slice(8, 16), slice(0, 32))           # tile row 1, tile column 0 of image 0
    for y, x in ((7, 10), (12, 32)):                 # in the tile's halo, not in the tile
        other = base.clone()
        other[0, y, x] += 0.5
        _, _, (pb,) = _census_fwd(im, f, [other], [(h, w)], r, [1.0])
        assert not torch.equal(pa[tile], pb[tile]), (y, x)
        assert torch.equal(pa[1], pb[1])             # the other image is not touched


# ------------------------------------------------------------------------- 4. LossLayer ----
@functools.lru_cache(maxsize=None)
def _layer_ref(mode):
    """The LossLayer case of ``mode`` and, in float64, the reference masks and the three terms
    with their d(flow): masked photometric, masked census (r = 3), smoothness (alpha 10)."""
    batch, flows = O.layer_case(mode)
    b = f64(batch)
    masks = O.masks([f64(f) for f in flows], mode)
    terms = []
    for fn in (lambda fo: O.photometric(b, fo, masks), lambda fo: O.census(b, fo, 3, masks),
               lambda fo: ref_smooth(b, fo, 10.0)):
        fo = [f64(f).requires_grad_(True) for f in flows]
        v = fn(fo)
        terms.append((v.item(), torch.autograd.grad(v, fo)))
    return batch, flows, masks, terms


@pytest.mark.parametrize("mode", ["border", "fb"])
def test_occlusion_masks_op(mode):
    """ops.occlusion_masks on the pyramid of the LossLayer case (alpha2 / 4^(s+1) per level):
    the reference masks on every pixel, as plain tensors without autograd."""
    from optical_flow_amd import ops
    _, flows, masks, _ = _layer_ref(mode)
    got = ops.occlusion_masks([dev(f).requires_grad_(True) for f in flows], mode)
    for f, m, want in zip(flows, got, masks):
        assert m.shape == f.shape[:3] and m.dtype == torch.float32 and not m.requires_grad
        print(mode, tuple(m.shape), "valid", m.mean().item())
        assert torch.equal(m.cpu().double(), want)


LAYERS = {"photometric": (dict(), (1.0, 0.0, 0.0)),
          "census": (dict(census_weight=1.0, photometric_weight=0.0), (0.0, 1.0, 0.0)),
          "all_three": (dict(smoothness_weight=0.2, edge_alpha=10, census_weight=0.5,
                             photometric_weight=0.5), (0.5, 0.5, 0.2))}


@pytest.mark.parametrize("which", list(LAYERS))
@pytest.mark.parametrize("mode", ["border", "fb"])
def test_loss_layer_with_occlusion(mode, which):
    """LossLayer(occlusion=mode): the loss and every d(flow) against the reference composition
    with the (detached) reference masks."""
    from optical_flow_amd.loss import LossLayer
    batch, flows, _, terms = _layer_ref(mode)
    kw, mix = LAYERS[which]
    want = sum(c * t[0] for c, t in zip(mix, terms))
    grads = [sum(c * t[1][s] for c, t in zip(mix, terms)) for s in range(len(flows))]
    fd = [dev(f).requires_grad_(True) for f in flows]
    loss = LossLayer(warp_convention="image", occlusion=mode, **kw)(dev(batch), fd)
    loss.backward()
    errs = [rel_l2(f.grad, g) for f, g in zip(fd, grads)]
    print(mode, which, loss.item(), want, "d(flow)", errs)
    assert loss.shape == () and _rel(loss.item(), want) < REL_TOL
    assert max(errs) < REL_TOL, errs


@pytest.mark.parametrize("dx,dy", [(16, -16), (-32, 16)])
def test_true_flow_minimises_the_masked_loss(dx, dy):
    """A pure translation scored with its true flow: with the border mask the photometric loss
    is < 1e-6, unmasked it is > 0.05 (all of it from samples outside the frame)."""
    from optical_flow_amd.loss import LossLayer
    pair = dev(shifted_pair(64, 96, dx, dy).float())
    flows = [dev(f.float()) for f in true_flows(64, 96, dx, dy)]
    masked = LossLayer(occlusion="border", warp_convention="image")(pair, flows).item()
    plain = LossLayer(occlusion="none", warp_convention="image")(pair, flows).item()
    print("masked", masked, "unmasked", plain)
    assert 0.0 <= masked < 1e-6 and plain > 0.05


# ------------------------------------------------------------------------------ 5. step ----
NET_SEED, BATCH_SEED = 0, 1236


def _fb_trainer():
    from optical_flow_amd.loss import LossLayer
    from optical_flow_amd.model import build_flow_net
    from optical_flow_amd.train import Trainer
    net = build_flow_net(64, 64, seed=NET_SEED, levels=4, warp_convention="image")
    layer = LossLayer(0.2, 10, census_weight=1.0, photometric_weight=0.0,
                      warp_convention="image", occlusion="fb")
    return Trainer(net, loss_layer=layer)


def _batch():
    from optical_flow_amd.data import synthetic_batch
    return dev(torch.from_numpy(synthetic_batch(2, 64, 64, seed=BATCH_SEED)))


def test_fb_train_step():
    """Trainer.train_step with occlusion="fb" (census + smoothness, image convention) at
    64 x 64, B = 2: the net runs on the doubled batch, the loss is finite, the returned flows
    have batch B; twice from the same state: loss and parameters bitwise equal."""
    batch = _batch()
    res = []
    for _ in range(2):
        trainer = _fb_trainer()
        loss, flows = trainer.train_step(batch)
        torch.cuda.synchronize()
        assert torch.isfinite(loss).all()
        assert [tuple(f.shape) for f in flows] == [(2, 64 >> (s + 1), 64 >> (s + 1), 2)
                                                   for s in range(4)]
        assert all(torch.isfinite(f).all() for f in flows)
        store = trainer.flow_net.store
        assert torch.isfinite(store.grad_arena).all() and store.grad_arena.abs().max() > 0
        res.append((loss.clone(), store.arena.clone()))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])


def test_fb_step_captures():
    """trainer.graphed captures the fb step (the doubled batch is formed on the device inside
    the capture); a replay's loss equals the eager step's on the same weights and batch, and
    the replay returns forward flows of batch B."""
    from test_gpu_graph import _sync_state
    batch = _batch()
    gt, eager = _fb_trainer(), _fb_trainer()
    step = gt.graphed(batch.clone(), warmup=1)
    _sync_state(eager, gt)
    le, fe = eager.train_step(batch)
    lg, fg = step(batch)
    torch.cuda.synchronize()
    print("replay loss", float(lg), "eager", float(le))
    assert _rel(float(lg), float(le)) < REL_TOL
    assert [tuple(f.shape) for f in fg] == [tuple(f.shape) for f in fe]
    assert fg[0].shape[0] == 2
    assert max(rel_l2(a, b) for a, b in zip(fg, fe)) < REL_TOL
