"""The census data term (DESIGN.md "Census term"; include/oflow.h of_census_*): the kernels
through the C ABI, known answers, ops.census_loss, LossLayer(census_weight, census_radius,
photometric_weight), a whole train step and the train command, against the float64
restatement of the definition in tests/census_ref.py (oracle.ref_flow's warp and resize, its
photometric loss for the other data term, test_gpu_smooth_loss's reference for the
regulariser).  Tolerance: the project's REL_TOL (rel_l2 on gradients, relative error on
scalars); on the shapes of the ABI test a float32 torch evaluation of the reference is within
2e-6 (value) and 5e-5 (d(flow)) of float64."""
import ctypes as C
import functools

import pytest
import torch

import census_ref
from helpers import REL_TOL, dev, f64, rel_l2, rng_tensor
from oracle import ref_flow as R
from test_gpu_smooth_loss import ref_smooth

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return abs(a - b) / abs(b)


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def _ptrs(ts):
    return _arr(C.c_void_p, [t.data_ptr() for t in ts])


def _fwd(imgs, flows, n, levels, r, coefs, planes=True):
    """of_census_fwd_multi -> (per-level partial-slice sums in float64 on the host, the
    partials, the d C_l / d flow planes or None)."""
    from optical_flow_amd import _lib, ops
    from optical_flow_amd._lib import call
    nparts = [_lib.lib().of_census_partials(n, h, w) for h, w in levels]
    parts = torch.full((sum(nparts),), float("nan"), device="cuda")
    pl = [torch.full((n, h, w, 2), float("nan"), device="cuda") for h, w in levels] \
        if planes else None
    assert all(_lib.lib().of_census_workspace_floats(n, h, w) == 0 for h, w in levels)
    call("of_census_fwd_multi", _ptrs(imgs), _ptrs(flows), n,
         _arr(C.c_int, [h for h, _ in levels]), _arr(C.c_int, [w for _, w in levels]),
         len(levels), r, _arr(C.c_float, coefs), None, _ptrs(pl) if planes else None,
         ops._ptr(parts), ops._stream())
    torch.cuda.synchronize()
    sums, o = [], 0
    for k in nparts:
        sums.append(parts[o:o + k].double().sum().item())
        o += k
    return sums, parts, pl


def _bwd(planes, n, levels, coefs, dloss, outs, ld, accumulate):
    from optical_flow_amd import ops
    from optical_flow_amd._lib import call
    L = len(levels)
    call("of_census_bwd_multi", _ptrs(planes), n, _arr(C.c_int, [h for h, _ in levels]),
         _arr(C.c_int, [w for _, w in levels]), L, _arr(C.c_float, coefs), ops._ptr(dloss),
         _ptrs(outs), _arr(C.c_int, [ld] * L), accumulate, ops._stream())
    torch.cuda.synchronize()


# ------------------------------------------------------------ 1. kernels through the ABI ----
# no pairs / a single row / an image smaller than the window; under one 8 x 32 tile, ragged in
# both directions, one pixel past tile edges; several tiles per image
CASES = [([(1, 1), (1, 9), (5, 3), (2, 2)], 3),
         ([(13, 21), (40, 57), (33, 65)], 3), ([(13, 21), (40, 57), (33, 65)], 2),
         ([(96, 128)], 1), ([(96, 128)], 3)]
N = 2


@functools.lru_cache(maxsize=None)
def _abi_case(idx):
    """Inputs and the float64 reference of CASES[idx]: per level C_l and d C_l / d flow."""
    levels, r = CASES[idx]
    flows = [rng_tensor((N, h, w, 2), 300 + i, scale=3.0) for i, (h, w) in enumerate(levels)]
    imgs = [rng_tensor((N, h, w, 6), 400 + i, lo=-0.5, hi=0.6) for i, (h, w) in enumerate(levels)]
    cs, grads = [], []
    for f, im in zip(flows, imgs):
        fo = f64(f).requires_grad_(True)
        c = census_ref.level_sum(*census_ref.gray_pair(f64(im), fo), r)
        grads.append(torch.autograd.grad(c, fo)[0] if c.requires_grad else torch.zeros_like(fo))
        cs.append(c.item())
    return flows, imgs, cs, grads


@pytest.mark.parametrize("with_dloss", [False, True])
@pytest.mark.parametrize("idx", range(len(CASES)), ids=lambda i: "case%d_r%d" % (i, CASES[i][1]))
def test_census_kernels_abi(idx, with_dloss):
    """Each level's partial slice is coefs[l] * C_l (exactly 0 for a 1 x 1 level); the plane is
    d C_l / d flow of autograd; the backward scales it at stride 2, at stride 4 overwriting
    (padding untouched, values bitwise those of stride 2) and at stride 4 accumulating; without
    planes the partials are bitwise the same.  Flows of scale 3: many samples clamp."""
    levels, r = CASES[idx]
    L = len(levels)
    flows, imgs, cs, grads = _abi_case(idx)
    fd, idv = [dev(f) for f in flows], [dev(i) for i in imgs]
    coefs = [0.3 + 0.1 * l for l in range(L)]
    sums, parts, planes = _fwd(idv, fd, N, levels, r, coefs)
    sums0, parts0, _ = _fwd(idv, fd, N, levels, r, coefs, planes=False)
    assert torch.equal(parts, parts0)
    for l, (h, w) in enumerate(levels):
        want = coefs[l] * cs[l]
        ep = rel_l2(planes[l], grads[l])
        print("level", (h, w), "r", r, "value", sums[l], want, "plane rel_l2 %.2e" % ep)
        if (h, w) == (1, 1):
            assert sums[l] == 0.0 and want == 0.0 and (planes[l] == 0).all()
        else:
            assert _rel(sums[l], want) < REL_TOL
        assert ep < REL_TOL
    g = 1.75 if with_dloss else 1.0
    dloss = torch.tensor([g], device="cuda") if with_dloss else None
    # stride 2, overwrite (prefilled with NaN: every element is written)
    d2 = [torch.full((N, h, w, 2), float("nan"), device="cuda") for h, w in levels]
    _bwd(planes, N, levels, coefs, dloss, d2, 2, 0)
    # stride 4, overwrite into buffers prefilled with 7.0
    d4 = [torch.full((N, h, w, 4), 7.0, device="cuda") for h, w in levels]
    _bwd(planes, N, levels, coefs, dloss, d4, 4, 0)
    # stride 4, accumulate onto 7.0
    a4 = [torch.full((N, h, w, 4), 7.0, device="cuda") for h, w in levels]
    _bwd(planes, N, levels, coefs, dloss, a4, 4, 1)
    for l, (h, w) in enumerate(levels):
        want = grads[l] * (coefs[l] * g)
        e2, e4 = rel_l2(d2[l], want), rel_l2(d4[l][..., :2], want)
        ea = rel_l2(a4[l][..., :2], want + 7.0)
        print("level", (h, w), "d(flow) rel_l2: ld2 %.2e ld4 %.2e accumulate %.2e" % (e2, e4, ea))
        assert e2 < REL_TOL and e4 < REL_TOL and ea < REL_TOL
        assert torch.equal(d2[l], d4[l][..., :2])
        # the accumulating form adds the same fp32 gradient to what was there
        assert torch.equal(a4[l][..., :2], d4[l][..., :2] + 7.0)
        assert (d4[l][..., 2:] == 7.0).all() and (a4[l][..., 2:] == 7.0).all()


# ---------------------------------------------------------------------- 2. known answers ----
def _transposed_pair(n, s, offset):
    i1 = rng_tensor((n, s, s, 3), 21, lo=-0.5, hi=0.6)
    return torch.cat([i1, i1.transpose(1, 2) + offset], -1)


def test_identity_case():
    """Zero flow samples image 2 transposed (P1): with image 2 = image 1 transposed the warped
    image is image 1 bit for bit; value exactly 0 and gradient exactly 0 (37 x 37: two tile
    columns, five tile rows)."""
    n, s = 2, 37
    img, f = dev(_transposed_pair(n, s, 0.0)), torch.zeros(n, s, s, 2, device="cuda")
    sums, _, planes = _fwd([img], [f], n, [(s, s)], 3, [1.0])
    assert sums[0] == 0.0
    assert (planes[0] == 0).all()


def test_offset_case():
    """+0.125 on image 2: the photometric L1 is 0.125, the census mean stays < 1e-9."""
    from optical_flow_amd import _lib, ops
    from optical_flow_amd._lib import call
    n, s = 2, 37
    img, f = dev(_transposed_pair(n, s, 0.125)), torch.zeros(n, s, s, 2, device="cuda")
    sums, _, _ = _fwd([img], [f], n, [(s, s)], 3, [1.0])
    parts = torch.empty(_lib.lib().of_photo_l1_partials(n, s, s), device="cuda")
    call("of_photo_l1_fwd_multi", _ptrs([img]), _ptrs([f]), n, _arr(C.c_int, [s]),
         _arr(C.c_int, [s]), 1, ops._ptr(parts), ops._stream())
    l1 = parts.double().sum().item() / (n * s * s * 3)
    print("census mean", sums[0] / (n * s * s), "photometric", l1)
    assert 0.0 <= sums[0] / (n * s * s) < 1e-9
    assert _rel(l1, 0.125) < REL_TOL


def test_no_pair_across_images():
    """Two images, each constant, with different constants and different image-1 / image-2
    offsets: every pair inside an image has e = 0, so the value is exactly 0; a pair taken
    across an image boundary (or a row end wrapping into the next image) would show.  Square
    images and zero flow: every bilinear weight is then exactly 0 or 1 (the zero-flow warp of
    an h != w image extrapolates past the shorter side with weights like -31 and 32, whose
    rounding makes a constant image's warp only nearly constant)."""
    n, h, w = 2, 37, 37
    img = torch.empty(n, h, w, 6)
    img[0, ..., :3], img[0, ..., 3:] = 0.1, 0.3
    img[1, ..., :3], img[1, ..., 3:] = -0.2, 0.25
    f = torch.zeros(n, h, w, 2, device="cuda")
    for r in (1, 3):
        sums, _, planes = _fwd([dev(img)], [f], n, [(h, w)], r, [1.0])
        assert sums[0] == 0.0 and (planes[0] == 0).all()


# ------------------------------------------------ 3./4. ops.census_loss, LossLayer ----
SIZES = [(2, 64, 96), (1, 48, 80), (3, 80, 112)]


def _pyramid_case(size):
    from optical_flow_amd.data import synthetic_batch
    n, H, W = size
    batch = torch.from_numpy(synthetic_batch(n, H, W, seed=5))
    flows = [rng_tensor((n, H >> (s + 1), W >> (s + 1), 2), 50 + s, scale=2.0) for s in range(4)]
    return batch, flows


def _check(loss_d, fd, loss_o, fo, what):
    errs = [rel_l2(a.grad, b.grad) for a, b in zip(fd, fo)]
    print(what, loss_d.item(), loss_o.item(), "d(flow)", errs)
    assert loss_d.shape == () and _rel(loss_d.item(), loss_o.item()) < REL_TOL
    assert max(errs) < REL_TOL, errs


@pytest.mark.parametrize("size", SIZES)
def test_census_loss_op(size):
    """ops.census_loss: the value and all four d(flow)."""
    from optical_flow_amd import ops
    batch, flows = _pyramid_case(size)
    fo = [f64(f).requires_grad_(True) for f in flows]
    co = census_ref.census(f64(batch), fo, 3)
    co.backward()
    fd = [dev(f).requires_grad_(True) for f in flows]
    cd = ops.census_loss(dev(batch), fd)
    cd.backward()
    _check(cd, fd, co, fo, "census")


@pytest.mark.parametrize("size", SIZES)
def test_loss_layer_with_census(size):
    """LossLayer(census_weight=1.0): photometric + census, loss and every d(flow)."""
    from optical_flow_amd.loss import LossLayer
    batch, flows = _pyramid_case(size)
    fo = [f64(f).requires_grad_(True) for f in flows]
    lo = R.photometric_loss(f64(batch), fo) + census_ref.census(f64(batch), fo, 3)
    lo.backward()
    fd = [dev(f).requires_grad_(True) for f in flows]
    ld = LossLayer(census_weight=1.0)(dev(batch), fd)
    ld.backward()
    _check(ld, fd, lo, fo, "loss")


def test_loss_layer_all_three_terms():
    """LossLayer(0.2, 10, census_weight=0.5, photometric_weight=0.5): the weighted sum of the
    three references."""
    from optical_flow_amd.loss import LossLayer
    batch, flows = _pyramid_case((2, 64, 96))
    fo = [f64(f).requires_grad_(True) for f in flows]
    b = f64(batch)
    lo = (0.5 * R.photometric_loss(b, fo) + 0.5 * census_ref.census(b, fo, 3) +
          0.2 * ref_smooth(b, fo, 10.0))
    lo.backward()
    fd = [dev(f).requires_grad_(True) for f in flows]
    ld = LossLayer(0.2, 10, census_weight=0.5, photometric_weight=0.5)(dev(batch), fd)
    ld.backward()
    _check(ld, fd, lo, fo, "loss")


def test_census_only_launches_no_photometric_kernel(monkeypatch):
    """photometric_weight = 0: census (+ smoothness) alone, the photometric entry points are
    not called; census radius 2."""
    from optical_flow_amd import ops
    from optical_flow_amd.loss import LossLayer
    batch, flows = _pyramid_case((2, 64, 96))
    fo = [f64(f).requires_grad_(True) for f in flows]
    b = f64(batch)
    lo = 0.7 * census_ref.census(b, fo, 2) + 0.2 * ref_smooth(b, fo, 10.0)
    lo.backward()
    called = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    fd = [dev(f).requires_grad_(True) for f in flows]
    ld = LossLayer(0.2, 10, census_weight=0.7, census_radius=2,
                   photometric_weight=0.0)(dev(batch), fd)
    ld.backward()
    assert "of_census_fwd_multi" in called and "of_census_bwd_multi" in called
    assert not [c for c in called if c.startswith("of_photo_l1")]
    _check(ld, fd, lo, fo, "loss")


# ------------------------------------------------------------ 5./6. through the model ----
# Net seed 0 and batch seed 1236 at 64 x 64, B = 2 (the smoothness test's case): the float32
# oracle's step with the census term is within 7e-8 (loss) and 5.7e-5 (worst parameter
# gradient) of its float64 step; with five levels 5.2e-8, 6.3e-5 and 9.5e-5 (worst d(flow)).
# photometric_weight stays 1: the census-only five-level case reads 2.1e-4 in the float32
# oracle, 5x from REL_TOL.
NET_SEED, BATCH_SEED = 0, 1236


def _oracle_step(batch, vals, levels, dtype=torch.float64):
    from optical_flow_amd.params import encoder_blocks
    p = {k: torch.tensor(v).to(dtype) for k, v in vals.items()}
    tr = {k: v.requires_grad_(True) for k, v in p.items()
          if not k.endswith(("moving_mean", "moving_variance"))}
    b = torch.tensor(batch).to(dtype)
    flows = R.flow_net(b, p, list(encoder_blocks(levels)))
    for f in flows:
        f.retain_grad()
    loss = R.photometric_loss(b, flows) + census_ref.census(b, flows, 3)
    loss.backward()
    return loss.detach(), flows, {k: v.grad for k, v in tr.items()}


def _model_case(levels=4):
    from optical_flow_amd.data import synthetic_batch
    from optical_flow_amd.loss import LossLayer
    from optical_flow_amd.model import build_flow_net
    from optical_flow_amd.train import Trainer
    net = build_flow_net(64, 64, seed=NET_SEED, levels=levels)
    vals = net.store.state()
    batch = synthetic_batch(2, 64, 64, seed=BATCH_SEED)
    return net, vals, batch, Trainer(net, loss_layer=LossLayer(census_weight=1.0))


def test_train_step_with_census():
    """One Trainer.train_step with LossLayer(census_weight=1.0) at 64 x 64, B = 2, fp32: the
    flows' gradients travel through the FlowGrad buffers (photometric write, census add, then
    upscale_flow's add).  Loss and every parameter gradient against the float64 oracle."""
    net, vals, batch, trainer = _model_case()
    loss_o, _, grads_o = _oracle_step(batch, vals, 4)
    loss, _ = trainer.train_step(dev(torch.from_numpy(batch)))
    torch.cuda.synchronize()
    grads = net.store.grads()
    assert set(grads) == set(grads_o)
    errs = sorted(((rel_l2(g, grads_o[k]), k) for k, g in grads.items()), reverse=True)
    print("loss", loss.item(), loss_o.item(), "worst gradients", errs[:4])
    assert _rel(loss.item(), loss_o.item()) < REL_TOL
    assert errs[0][0] < REL_TOL, errs[0]


def test_five_levels_with_census():
    """levels=5 at 64 x 64 (five flows, the coarsest 2 x 2: smaller than the window; six
    groups in the loss's final sum): the loss value and the flows' gradients."""
    from optical_flow_amd.loss import LossLayer
    net, vals, batch, _ = _model_case(levels=5)
    loss_o, flows_o, _ = _oracle_step(batch, vals, 5)
    bd = dev(torch.from_numpy(batch))
    net.store.zero_grad()
    flows = net(bd)
    assert len(flows) == 5 and flows[-1].shape == (2, 2, 2, 2)
    for f in flows:
        f.retain_grad()
    loss = LossLayer(census_weight=1.0)(bd, flows)
    loss.backward()
    torch.cuda.synchronize()
    errs = [rel_l2(f.grad, fo.grad) for f, fo in zip(flows, flows_o)]
    print("loss", loss.item(), loss_o.item(), "d(flow)", errs)
    assert _rel(loss.item(), loss_o.item()) < REL_TOL
    assert max(errs) < REL_TOL, errs


def test_train_step_with_census_is_deterministic():
    """The step of test_train_step_with_census twice from the same state: losses and all
    gradients bitwise equal (no atomics in the new kernels)."""
    res = []
    for _ in range(2):
        net, vals, batch, trainer = _model_case()
        loss, _ = trainer.train_step(dev(torch.from_numpy(batch)))
        torch.cuda.synchronize()
        res.append((loss.clone(), net.store.grad_arena.clone()))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])


# ------------------------------------------------------------------ 7. default unchanged ----
@pytest.mark.parametrize("args", [(), (0.2, 10)], ids=["photometric", "smoothness"])
def test_default_dispatch_is_unchanged(args):
    """LossLayer() is bitwise ops.photometric_loss and LossLayer(0.2, 10) bitwise
    ops.flow_loss(..., 0.2, 10), value and d(flow): with the new arguments at their defaults
    no new code runs."""
    from optical_flow_amd import ops
    from optical_flow_amd.loss import LossLayer
    batch, flows = _pyramid_case((2, 64, 96))
    bd = dev(batch)
    direct = (lambda b, f: ops.flow_loss(b, f, 0.2, 10)) if args else ops.photometric_loss
    layer = LossLayer(*args)
    assert layer.census_weight == 0.0 and layer.photometric_weight == 1.0
    out = []
    for fn in (layer, direct):
        fd = [dev(f).requires_grad_(True) for f in flows]
        loss = fn(bd, fd)
        loss.backward()
        out.append((loss.detach(), [f.grad for f in fd]))
    assert torch.equal(out[0][0], out[1][0])
    for a, b in zip(out[0][1], out[1][1]):
        assert torch.equal(a, b)


# --------------------------------------------------------------------- 8. train command ----
def test_train_command_logs_the_settings(tmp_path):
    """python -m optical_flow_amd.train --census-weight 1 --census-radius 2 --log: the JSONL
    starts with a header record holding the three values (and the existing keys), then one
    finite record per step."""
    import json
    from optical_flow_amd.train import main
    log = tmp_path / "log.jsonl"
    main(["--height", "64", "--width", "64", "--batch", "1", "--steps", "2",
          "--census-weight", "1", "--census-radius", "2", "--log", str(log)])
    recs = [json.loads(l) for l in open(log).read().splitlines() if l]
    head = recs[0]
    assert (head["census_weight"], head["census_radius"], head["photometric_weight"]) == \
        (1.0, 2, 1.0)
    assert head["header"] is True and head["smoothness_weight"] == 0.0 and \
        head["edge_alpha"] == 0.0
    assert "step" not in head and [r["step"] for r in recs[1:]] == [0, 1]
    assert all(r["loss"] == r["loss"] and abs(r["loss"]) < 1e3 for r in recs[1:])
