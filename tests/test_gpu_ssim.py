"""The SSIM data term (DESIGN.md "SSIM term"; include/oflow.h of_ssim_*): the kernel through
the C ABI, known answers, centre weights, ops.ssim_loss, LossLayer(ssim_weight) alone and mixed
with the other terms and the occlusion masks, the off switch, and a whole train step, against
the float64 restatement of the definition in tests/ssim_ref.py.  Tolerance: the project's
REL_TOL (rel_l2 on gradients, relative error on scalars); tests/test_ssim_host.py shows a
float32 evaluation of the reference within REL_TOL / 10 of float64 on every input used here
(tests/ssim_cases.py)."""
import ctypes as C
import functools

import pytest
import torch

import occlusion_ref as O
import ssim_cases as SC
import ssim_ref
from helpers import REL_TOL, dev, f64, rel_l2
from oracle import ref_flow as R
from test_gpu_smooth_loss import ref_smooth

pytestmark = pytest.mark.gpu

CV = {"reference": 0, "image": 1}
N = SC.N


def _rel(a, b):
    return abs(a - b) / abs(b)


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def _ptrs(ts):
    return _arr(C.c_void_p, [t.data_ptr() if t is not None else None for t in ts])


def _counts(n, levels):
    from optical_flow_amd import _lib
    return [_lib.lib().of_ssim_partials(n, h, w) for h, w in levels]


def _fwd(imgs, flows, n, levels, coefs, cv, weights=None, planes=True):
    """of_ssim_fwd_multi, one launch -> (per-level partial-slice sums in float64 on the host,
    the partials, the d SSIM_l / d flow planes or None).  Outputs are prefilled with NaN."""
    from optical_flow_amd import ops
    from optical_flow_amd._lib import call
    parts = torch.full((sum(_counts(n, levels)),), float("nan"), device="cuda")
    pl = [torch.full((n, h, w, 2), float("nan"), device="cuda") for h, w in levels] \
        if planes else None
    call("of_ssim_fwd_multi", _ptrs(imgs), _ptrs(flows),
         _ptrs(weights) if weights is not None else None, n,
         _arr(C.c_int, [h for h, _ in levels]), _arr(C.c_int, [w for _, w in levels]),
         len(levels), _arr(C.c_float, coefs), _ptrs(pl) if planes else None, ops._ptr(parts),
         CV[cv], ops._stream())
    torch.cuda.synchronize()
    sums, o = [], 0
    for k in _counts(n, levels):
        sums.append(parts[o:o + k].double().sum().item())
        o += k
    return sums, parts, pl


def _bwd(planes, n, levels, coefs, dloss, outs, ld, accumulate):
    from optical_flow_amd import ops
    from optical_flow_amd._lib import call
    L = len(levels)
    call("of_ssim_bwd_multi", _ptrs(planes), n, _arr(C.c_int, [h for h, _ in levels]),
         _arr(C.c_int, [w for _, w in levels]), L, _arr(C.c_float, coefs), ops._ptr(dloss),
         _ptrs(outs), _arr(C.c_int, [ld] * L), accumulate, ops._stream())
    torch.cuda.synchronize()


def _coefs(levels, n=N):
    """The term's own normalisers: 1 / (L n (h-2)(w-2) 3), 0 for a level without a window."""
    return [ssim_ref.level_coef(n, h, w, len(levels)) for h, w in levels]


def _windowless(h, w):
    return h < 3 or w < 3


# ------------------------------------------------------------ 1. kernel through the ABI ----
@pytest.mark.parametrize("with_dloss", [False, True], ids=["nodloss", "dloss"])
@pytest.mark.parametrize("cv", SC.CONVENTIONS)
def test_ssim_kernels_abi(cv, with_dloss):
    """All six levels in one launch, n = 3.  Each level's partial slice is coefs[l] * SSIM_l,
    their sum the loss; the plane is d SSIM_l / d flow of float64 autograd, every element
    written (NaN prefill) and exactly 0 on levels without a window; without planes the partials
    are bitwise the same.  The backward scales the plane at row stride 2, at stride 4
    overwriting (padding untouched, values bitwise those of stride 2) and at stride 4
    accumulating."""
    levels = SC.LEVELS
    imgs, flows = SC.textured()
    ref = SC.level_reference("textured", cv)
    idv, fd = [dev(i) for i in imgs], [dev(f) for f in flows]
    coefs = _coefs(levels)
    sums, parts, planes = _fwd(idv, fd, N, levels, coefs, cv)
    _, parts0, _ = _fwd(idv, fd, N, levels, coefs, cv, planes=False)
    assert torch.equal(parts, parts0)
    for l, (h, w) in enumerate(levels):
        want = coefs[l] * ref[l][0]
        assert not torch.isnan(planes[l]).any(), "plane of %s not fully written" % ((h, w),)
        ep = rel_l2(planes[l], ref[l][1])
        print(cv, "level", (h, w), "value", sums[l], want, "plane rel_l2 %.2e" % ep)
        if _windowless(h, w):
            assert sums[l] == 0.0 and want == 0.0 and (planes[l] == 0).all()
        else:
            assert _rel(sums[l], want) < REL_TOL
        assert ep < REL_TOL
    loss, want = parts.double().sum().item(), sum(c * r[0] for c, r in zip(coefs, ref))
    print(cv, "loss", loss, want)
    assert _rel(loss, want) < REL_TOL
    g = 1.75 if with_dloss else 1.0
    dloss = torch.tensor([g], device="cuda") if with_dloss else None
    d2 = [torch.full((N, h, w, 2), float("nan"), device="cuda") for h, w in levels]
    _bwd(planes, N, levels, coefs, dloss, d2, 2, 0)
    d4 = [torch.full((N, h, w, 4), 7.0, device="cuda") for h, w in levels]
    _bwd(planes, N, levels, coefs, dloss, d4, 4, 0)
    a4 = [torch.full((N, h, w, 4), 7.0, device="cuda") for h, w in levels]
    _bwd(planes, N, levels, coefs, dloss, a4, 4, 1)
    for l, (h, w) in enumerate(levels):
        want = ref[l][1] * (coefs[l] * g)
        e2, e4 = rel_l2(d2[l], want), rel_l2(d4[l][..., :2], want)
        ea = rel_l2(a4[l][..., :2], want + 7.0)
        print("level", (h, w), "d(flow) rel_l2: ld2 %.2e ld4 %.2e accumulate %.2e" % (e2, e4, ea))
        assert e2 < REL_TOL and e4 < REL_TOL and ea < REL_TOL
        assert torch.equal(d2[l], d4[l][..., :2])
        assert torch.equal(a4[l][..., :2], d4[l][..., :2] + 7.0)
        assert (d4[l][..., 2:] == 7.0).all() and (a4[l][..., 2:] == 7.0).all()


@pytest.mark.parametrize("cv", SC.CONVENTIONS)
def test_low_texture(cv):
    """Intensities 0.8 + 0.003 U (tests/ssim_cases.py says why not 0.002), sigma ~ 7e-7 beside
    mu^2 ~ 0.64: the case an uncentred variance E[x^2] - mu^2 fails in float32 (1.1e-3 to
    2.7e-3 off in the value on these inputs; the centred float32 reference 5e-7).  Value and
    plane at REL_TOL."""
    levels = SC.LOW_LEVELS
    imgs, flows = SC.low_texture()
    ref = SC.level_reference("low", cv)
    coefs = _coefs(levels)
    sums, _, planes = _fwd([dev(i) for i in imgs], [dev(f) for f in flows], N, levels, coefs, cv)
    for l, (h, w) in enumerate(levels):
        ev, ep = _rel(sums[l], coefs[l] * ref[l][0]), rel_l2(planes[l], ref[l][1])
        print(cv, "level", (h, w), "value rel %.2e plane rel_l2 %.2e" % (ev, ep))
        assert ev < REL_TOL and ep < REL_TOL


# ---------------------------------------------------------------------- 2. known answers ----
def _stored(value, shape):
    """An image whose intensity is ``value`` everywhere: value - mean_c stored."""
    return torch.full(shape + (3,), value) - torch.tensor(ssim_ref.MEANS, dtype=torch.float32)


@pytest.mark.parametrize("cv", SC.CONVENTIONS)
def test_constant_images(cv):
    """x = a, y = b everywhere, any flow (the warp of a constant is that constant): sigma = 0
    and the loss is (a-b)^2 / (2 (a^2 + b^2 + C1)), 0.027023 for 0.5 / 0.7."""
    levels = [(13, 21), (40, 57)]
    a, b = 0.5, 0.7
    imgs = [dev(torch.cat([_stored(a, (N, h, w)), _stored(b, (N, h, w))], -1)) for h, w in levels]
    flows = [dev(f) for f in SC.textured()[1][4:]]
    sums, parts, _ = _fwd(imgs, flows, N, levels, _coefs(levels), cv)
    want = (a - b) ** 2 / (2 * (a * a + b * b + ssim_ref.C1))
    loss = parts.double().sum().item()
    print(cv, "loss", loss, want)
    assert abs(want - 0.027023) < 5e-7 and _rel(loss, want) < REL_TOL


def test_identity():
    """Image 2 = image 1 with zero flow in the image convention: y is x bit for bit and the
    loss a few ulp of a ratio of equal sums at most."""
    levels = [(13, 21), (40, 57)]
    imgs = [dev(torch.cat([i[..., :3], i[..., :3]], -1)) for i in SC.textured()[0][4:]]
    flows = [torch.zeros(N, h, w, 2, device="cuda") for h, w in levels]
    _, parts, planes = _fwd(imgs, flows, N, levels, _coefs(levels), "image")
    loss = parts.double().sum().item()
    print("identity loss", loss)
    assert abs(loss) <= 1e-6


def test_no_window_across_images():
    """Changing image 1 of the batch (pictures and flow) leaves the partials of images 0 and 2
    bitwise as they were: no window reaches into a neighbouring image, no row end wraps."""
    levels = [(13, 21), (40, 57)]
    imgs, flows = [t[4:] for t in SC.textured()]
    coefs = _coefs(levels)
    _, p0, _ = _fwd([dev(i) for i in imgs], [dev(f) for f in flows], N, levels, coefs, "image")
    imgs2, flows2 = [i.clone() for i in imgs], [f.clone() for f in flows]
    for i, f in zip(imgs2, flows2):
        i[1] = i[1].flip(0) * 0.5 + 0.1
        f[1] = -f[1]
    _, p1, _ = _fwd([dev(i) for i in imgs2], [dev(f) for f in flows2], N, levels, coefs, "image")
    o = 0
    for k in _counts(N, levels):
        per = k // N
        a, b = p0[o:o + k].view(N, per), p1[o:o + k].view(N, per)
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
        assert not torch.equal(a[1], b[1])
        o += k


# ----------------------------------------------------------------------------- 3. weights ----
def test_weights_of_one_are_no_weights():
    """All-ones weights, a NULL array and NULL entries: bitwise-equal partials and planes."""
    levels = SC.LEVELS
    idv, fd = [[dev(t) for t in ts] for ts in SC.textured()]
    coefs = _coefs(levels)
    ones = [torch.ones(N, h, w, device="cuda") for h, w in levels]
    _, p_null, pl_null = _fwd(idv, fd, N, levels, coefs, "image")
    _, p_ones, pl_ones = _fwd(idv, fd, N, levels, coefs, "image", weights=ones)
    _, p_none, pl_none = _fwd(idv, fd, N, levels, coefs, "image", weights=[None] * len(levels))
    mixed = [o if l % 2 else None for l, o in enumerate(ones)]
    _, p_mix, pl_mix = _fwd(idv, fd, N, levels, coefs, "image", weights=mixed)
    for p, pl in ((p_ones, pl_ones), (p_none, pl_none), (p_mix, pl_mix)):
        assert torch.equal(p, p_null)
        assert all(torch.equal(a, b) for a, b in zip(pl, pl_null))


def test_zero_weights():
    """Weights of zero: every partial exactly 0.0 and a zero plane."""
    levels = SC.LEVELS
    idv, fd = [[dev(t) for t in ts] for ts in SC.textured()]
    zeros = [torch.zeros(N, h, w, device="cuda") for h, w in levels]
    _, parts, planes = _fwd(idv, fd, N, levels, _coefs(levels), "reference", weights=zeros)
    assert (parts == 0).all()
    assert all((pl == 0).all() for pl in planes)


@pytest.mark.parametrize("centre", [(8, 32), (7, 31), (1, 1), (38, 55), (16, 33)])
def test_single_weighted_centre(centre):
    """One centre of weight 1 in image 1 of the 40 x 57 level (on and next to tile edges, in
    the corners): the plane is non-zero only inside that centre's 3 x 3 window, and is non-zero
    there."""
    h, w = 40, 57
    img, flow = [dev(t[5]) for t in SC.textured()]
    wt = torch.zeros(N, h, w, device="cuda")
    wt[1, centre[0], centre[1]] = 1.0
    sums, _, planes = _fwd([img], [flow], N, [(h, w)], [1.0], "image", weights=[wt])
    inside = torch.zeros(N, h, w, dtype=torch.bool, device="cuda")
    inside[1, centre[0] - 1:centre[0] + 2, centre[1] - 1:centre[1] + 2] = True
    assert (planes[0][~inside] == 0).all()
    assert planes[0][inside].abs().sum() > 0 and sums[0] > 0


@pytest.mark.parametrize("cv", SC.CONVENTIONS)
def test_random_weights(cv):
    """Random non-negative weights on every pixel, so also on the centres a neighbouring tile
    holds in its halo: value and plane at REL_TOL."""
    levels = SC.LEVELS
    idv, fd = [[dev(t) for t in ts] for ts in SC.textured()]
    ref = SC.level_reference("textured", cv, True)
    wts = [dev(m) for m in SC.random_weights()]
    coefs = _coefs(levels)
    sums, _, planes = _fwd(idv, fd, N, levels, coefs, cv, weights=wts)
    for l, (h, w) in enumerate(levels):
        ep = rel_l2(planes[l], ref[l][1])
        print(cv, "level", (h, w), "value", sums[l], coefs[l] * ref[l][0], "plane %.2e" % ep)
        if _windowless(h, w):
            assert sums[l] == 0.0 and (planes[l] == 0).all()
        else:
            assert _rel(sums[l], coefs[l] * ref[l][0]) < REL_TOL
        assert ep < REL_TOL


# ------------------------------------------------------------------- 4. invalid arguments ----
def _null_entry(ts):
    return _ptrs([ts[0], None])


BAD = ["levels0", "levels9", "n0", "h0", "w0", "convention2", "convention-1", "img6s", "flows",
       "partials", "img6s[1]", "flows[1]"]


@pytest.mark.parametrize("bad", BAD)
def test_invalid_arguments(bad):
    """Every OF_EINVAL case returns 1 with the error naming the entry, and neither the
    partials nor the planes are touched."""
    from optical_flow_amd import _lib, ops
    levels = [(5, 3), (13, 21)]
    imgs = [dev(t) for t in SC.textured()[0][2:5:2]]
    flows = [dev(t) for t in SC.textured()[1][2:5:2]]
    assert [tuple(f.shape[1:3]) for f in flows] == levels
    parts = torch.full((sum(_counts(N, levels)),), 7.0, device="cuda")
    planes = [torch.full((N, h, w, 2), 7.0, device="cuda") for h, w in levels]
    a = dict(img6s=_ptrs(imgs), flows=_ptrs(flows), n=N, hs=_arr(C.c_int, [5, 13]),
             ws=_arr(C.c_int, [3, 21]), levels=2, partials=ops._ptr(parts), convention=0)
    a.update({"levels0": dict(levels=0), "levels9": dict(levels=9), "n0": dict(n=0),
              "h0": dict(hs=_arr(C.c_int, [5, 0])), "w0": dict(ws=_arr(C.c_int, [0, 21])),
              "convention2": dict(convention=2), "convention-1": dict(convention=-1),
              "img6s": dict(img6s=None), "flows": dict(flows=None), "partials": dict(partials=None),
              "img6s[1]": dict(img6s=_null_entry(imgs)),
              "flows[1]": dict(flows=_null_entry(flows))}[bad])
    lib = _lib.lib()
    st = lib.of_ssim_fwd_multi(a["img6s"], a["flows"], None, a["n"], a["hs"], a["ws"],
                               a["levels"], _arr(C.c_float, [1.0, 1.0]), _ptrs(planes),
                               a["partials"], a["convention"], ops._stream())
    torch.cuda.synchronize()
    assert st == 1 and b"of_ssim_fwd_multi" in lib.of_last_error()
    assert (parts == 7.0).all() and all((p == 7.0).all() for p in planes)


# ------------------------------------------------------- 5. ops.ssim_loss and LossLayer ----
@functools.lru_cache(maxsize=None)
def _pyramid_ref(levels, cv):
    """Float64 value and d(flow) of each term on the pyramid case: photometric, census r = 3,
    SSIM, smoothness (alpha 10)."""
    batch, flows = SC.pyramid_case(levels)
    b = f64(batch)
    terms = {}
    with SC.convention(cv):
        import census_ref
        for name, fn in (("photo", lambda fo: R.photometric_loss(b, fo)),
                         ("census", lambda fo: census_ref.census(b, fo, 3)),
                         ("ssim", lambda fo: ssim_ref.ssim(b, fo)),
                         ("smooth", lambda fo: ref_smooth(b, fo, 10.0))):
            fo = [f64(f).requires_grad_(True) for f in flows]
            v = fn(fo)
            g = torch.autograd.grad(v, fo, allow_unused=True)
            terms[name] = (v.item(), [torch.zeros_like(f) if x is None else x
                                      for x, f in zip(g, fo)])
    return batch, flows, terms


def _check_mix(loss, fd, terms, mix, what):
    want = sum(c * terms[k][0] for k, c in mix.items())
    grads = [sum(c * terms[k][1][s] for k, c in mix.items()) for s in range(len(fd))]
    errs = [rel_l2(f.grad, g) for f, g in zip(fd, grads)]
    print(what, loss.item(), want, "d(flow)", errs)
    assert loss.shape == () and _rel(loss.item(), want) < REL_TOL
    assert max(errs) < REL_TOL, errs
    for f, g in zip(fd, grads):
        if not g.any():
            assert not f.grad.any()


@pytest.mark.parametrize("levels", [4, 5])
@pytest.mark.parametrize("cv", SC.CONVENTIONS)
def test_ssim_loss_op(cv, levels):
    """ops.ssim_loss at 64 x 128, B = 2: the value and every d(flow); with five levels the
    fifth (2 x 4) has no window and its gradient is exactly zero."""
    from optical_flow_amd import ops
    batch, flows, terms = _pyramid_ref(levels, cv)
    fd = [dev(f).requires_grad_(True) for f in flows]
    loss = ops.ssim_loss(dev(batch), fd, convention=cv)
    loss.backward()
    _check_mix(loss, fd, terms, {"ssim": 1.0}, "ssim_loss %s %d" % (cv, levels))


MIXES = {
    "ssim_alone": (dict(photometric_weight=0.0, ssim_weight=1.0), {"ssim": 1.0}),
    "l1_ssim": (dict(photometric_weight=0.15, ssim_weight=0.85), {"photo": 0.15, "ssim": 0.85}),
    "all_four": (dict(smoothness_weight=0.2, edge_alpha=10, census_weight=0.5,
                      photometric_weight=0.5, ssim_weight=0.7),
                 {"photo": 0.5, "census": 0.5, "ssim": 0.7, "smooth": 0.2}),
}


@pytest.mark.parametrize("levels", [4, 5])
@pytest.mark.parametrize("mix", list(MIXES))
def test_loss_layer_with_ssim(mix, levels):
    """LossLayer(ssim_weight=...) alone, with L1 and with all four terms (five levels and four
    terms: 5 + 3 = 8 sum groups, the limit): loss and every d(flow)."""
    from optical_flow_amd.loss import LossLayer
    batch, flows, terms = _pyramid_ref(levels, "reference")
    kw, coef = MIXES[mix]
    fd = [dev(f).requires_grad_(True) for f in flows]
    loss = LossLayer(**kw)(dev(batch), fd)
    loss.backward()
    _check_mix(loss, fd, terms, coef, "%s %d" % (mix, levels))


@functools.lru_cache(maxsize=None)
def _masked_ref(mode):
    batch, flows = O.layer_case(mode)
    b = f64(batch)
    masks = O.masks([f64(f) for f in flows], mode)
    terms = {}
    with SC.convention("image"):
        for name, fn in (("photo", lambda fo: O.photometric(b, fo, masks)),
                         ("ssim", lambda fo: ssim_ref.ssim(b, fo, masks))):
            fo = [f64(f).requires_grad_(True) for f in flows]
            v = fn(fo)
            terms[name] = (v.item(), list(torch.autograd.grad(v, fo)))
    return batch, flows, terms


@pytest.mark.parametrize("mode", ["border", "fb"])
def test_loss_layer_with_ssim_and_occlusion(mode):
    """0.15 L1 + 0.85 SSIM with occlusion masks (the occlusion tests' conditioned flows): the
    mask weighs each window at its centre; loss and every d(flow)."""
    from optical_flow_amd.loss import LossLayer
    batch, flows, terms = _masked_ref(mode)
    fd = [dev(f).requires_grad_(True) for f in flows]
    loss = LossLayer(photometric_weight=0.15, ssim_weight=0.85, warp_convention="image",
                     occlusion=mode)(dev(batch), fd)
    loss.backward()
    _check_mix(loss, fd, terms, {"photo": 0.15, "ssim": 0.85}, "occlusion " + mode)


# --------------------------------------------------------------------------- 6. off switch ----
def _rows():
    """The dispatch rows of test_gpu_loss_paths.py that leave the SSIM term off."""
    from test_gpu_loss_paths import ROWS, SSF
    return [row for row, (_, fwd, _) in ROWS.items() if SSF not in fwd]


@pytest.mark.parametrize("row", _rows())
def test_off_switch(monkeypatch, row):
    """With ssim_weight = 0 no of_ssim* entry is called, forward or backward, by any dispatch
    row of test_gpu_loss_paths.py that has no SSIM term; with it on, the forward and the
    backward entry are."""
    from optical_flow_amd import ops
    from test_gpu_loss_paths import ROWS, _inputs
    batch, flows = _inputs()
    called = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    fd = [dev(f).requires_grad_(True) for f in flows]
    ROWS[row][0](ops, batch, fd).backward()
    torch.cuda.synchronize()
    assert called and not [c for c in called if c.startswith("of_ssim")]
    del called[:]
    fd = [dev(f).requires_grad_(True) for f in flows]
    ops.census_flow_loss(batch, fd, 0.0, photometric_weight=0.15, ssim_weight=0.85).backward()
    torch.cuda.synchronize()
    assert [c for c in called if c.startswith("of_ssim")] == ["of_ssim_fwd_multi",
                                                              "of_ssim_bwd_multi"]


# ---------------------------------------------------------------------------- 7. the step ----
NET_SEED, BATCH_SEED = 0, 1236


def _oracle_step(batch, vals, levels=4):
    from optical_flow_amd.params import encoder_blocks
    p = {k: torch.tensor(v).double() for k, v in vals.items()}
    tr = {k: v.requires_grad_(True) for k, v in p.items()
          if not k.endswith(("moving_mean", "moving_variance"))}
    b = torch.tensor(batch).double()
    flows = R.flow_net(b, p, list(encoder_blocks(levels)))
    loss = 0.15 * R.photometric_loss(b, flows) + 0.85 * ssim_ref.ssim(b, flows)
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in tr.items()}


def _trainer():
    from optical_flow_amd.loss import LossLayer
    from optical_flow_amd.model import build_flow_net
    from optical_flow_amd.train import Trainer
    net = build_flow_net(64, 64, seed=NET_SEED, levels=4)
    return net, Trainer(net, loss_layer=LossLayer(photometric_weight=0.15, ssim_weight=0.85))


def _batch():
    from optical_flow_amd.data import synthetic_batch
    return synthetic_batch(2, 64, 64, seed=BATCH_SEED)


def test_train_step_with_ssim():
    """One Trainer.train_step with 0.15 L1 + 0.85 SSIM at 64 x 64, B = 2, fp32: the flows'
    gradients travel through the FlowGrad buffers (photometric write, SSIM add, then
    upscale_flow's add).  Loss and every parameter gradient against the float64 oracle."""
    net, trainer = _trainer()
    batch = _batch()
    loss_o, grads_o = _oracle_step(batch, net.store.state())
    loss, _ = trainer.train_step(dev(torch.from_numpy(batch)))
    torch.cuda.synchronize()
    grads = net.store.grads()
    assert set(grads) == set(grads_o)
    errs = sorted(((rel_l2(g, grads_o[k]), k) for k, g in grads.items()), reverse=True)
    print("loss", loss.item(), loss_o.item(), "worst gradients", errs[:4])
    assert _rel(loss.item(), loss_o.item()) < REL_TOL
    assert errs[0][0] < REL_TOL, errs[0]


def test_train_step_with_ssim_is_deterministic():
    """The same step twice from the same state: loss and all gradients bitwise equal."""
    res = []
    for _ in range(2):
        net, trainer = _trainer()
        loss, _ = trainer.train_step(dev(torch.from_numpy(_batch())))
        torch.cuda.synchronize()
        res.append((loss.clone(), net.store.grad_arena.clone()))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])


def test_ssim_step_captures():
    """trainer.graphed captures the step with the SSIM term; a replay's loss equals the eager
    step's on the same weights and batch."""
    from optical_flow_amd import ops
    from test_gpu_graph import _sync_state
    batch = dev(torch.from_numpy(_batch()))
    # with the deterministic warp backward every reduction of the step has a fixed order, and
    # the replay computes what the eager step computes
    with ops.deterministic(True):
        (_, gt), (_, eager) = _trainer(), _trainer()
        step = gt.graphed(batch.clone(), warmup=1)
        _sync_state(eager, gt)
        le, fe = eager.train_step(batch)
        lg, fg = step(batch)
        torch.cuda.synchronize()
    print("replay loss", float(lg), "eager", float(le))
    assert float(lg) == float(le)
    assert all(torch.equal(a, b) for a, b in zip(fg, fe))
