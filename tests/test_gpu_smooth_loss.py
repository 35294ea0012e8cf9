"""The edge-aware flow smoothness term (include/oflow.h of_flow_smooth_*_multi):
the kernels through the C ABI, ops.flow_smoothness, LossLayer(smoothness_weight, edge_alpha)
and a whole train step, against a float64 reference written here from the definition

    rho(d)    = sqrt(d^2 + eps)
    wv[b,i,j] = exp(-alpha * mean_{c<3} |img[b,i,j,c] - img[b,i+1,j,c]|)     (wh: j+1)
    Sv        = sum wv * rho(f[b,i,j,c] - f[b,i+1,j,c]),  Sh likewise
    smooth_s  = Sv / (B (h-1) w 2) + Sh / (B h (w-1) 2),  smooth = mean_s smooth_s

with oracle.ref_flow's resize for the pyramid and its photometric loss for the other term.
Tolerance: the project's REL_TOL (rel_l2 on gradients, relative error on scalars)."""
import ctypes as C

import pytest
import torch

from helpers import REL_TOL, dev, f64, rel_l2, rng_tensor
from oracle import ref_flow as R

pytestmark = pytest.mark.gpu

EPS = 1e-4


# ---------------------------------------------------------------- float64 reference ----
def ref_level_sums(f, img, alpha, eps=EPS):
    """(Sv, Sh) of one level; img may be None when alpha == 0."""
    dv = f[:, :-1] - f[:, 1:]
    dh = f[:, :, :-1] - f[:, :, 1:]
    rv = torch.sqrt(dv * dv + eps)
    rh = torch.sqrt(dh * dh + eps)
    if alpha != 0:
        i1 = img[..., :3]
        rv = rv * torch.exp(-alpha * (i1[:, :-1] - i1[:, 1:]).abs().mean(-1, keepdim=True))
        rh = rh * torch.exp(-alpha * (i1[:, :, :-1] - i1[:, :, 1:]).abs().mean(-1, keepdim=True))
    return rv.sum(), rh.sum()


def ref_smooth(batch, flows, alpha, eps=EPS):
    H, W = batch.shape[1], batch.shape[2]
    total = batch.new_zeros(())
    for s, f in enumerate(flows):
        n, h, w, _ = f.shape
        img = None
        if alpha != 0:
            assert h == int(H / 2.0 ** (s + 1)) and w == int(W / 2.0 ** (s + 1))
            img = R.resize_bilinear(batch, h, w)
        sv, sh = ref_level_sums(f, img, alpha, eps)
        if h > 1:
            total = total + sv / (n * (h - 1) * w * 2)
        if w > 1:
            total = total + sh / (n * h * (w - 1) * 2)
    return total / len(flows)


def _rel(a, b):
    return abs(a - b) / abs(b)


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def _ptrs(ts):
    return _arr(C.c_void_p, [t.data_ptr() for t in ts])


def _fwd(flows, imgs, n, levels, alpha, cv, ch, eps=EPS):
    """of_flow_smooth_fwd_multi -> per-level partial-slice sums (float64, on the host)."""
    from optical_flow_amd import _lib, ops
    from optical_flow_amd._lib import call
    L = len(levels)
    nparts = [_lib.lib().of_flow_smooth_partials(n, h, w) for h, w in levels]
    parts = torch.full((sum(nparts),), float("nan"), device="cuda")
    call("of_flow_smooth_fwd_multi", _ptrs(imgs) if imgs is not None else None, _ptrs(flows), n,
         _arr(C.c_int, [h for h, _ in levels]), _arr(C.c_int, [w for _, w in levels]), L, alpha,
         eps, _arr(C.c_float, cv), _arr(C.c_float, ch), ops._ptr(parts), ops._stream())
    torch.cuda.synchronize()
    out, o = [], 0
    for k in nparts:
        out.append(parts[o:o + k].double().sum().item())
        o += k
    return out


def _bwd(flows, imgs, n, levels, alpha, cv, ch, dloss, outs, ld, accumulate, eps=EPS):
    from optical_flow_amd import ops
    from optical_flow_amd._lib import call
    L = len(levels)
    call("of_flow_smooth_bwd_multi", _ptrs(imgs) if imgs is not None else None, _ptrs(flows), n,
         _arr(C.c_int, [h for h, _ in levels]), _arr(C.c_int, [w for _, w in levels]), L, alpha,
         eps, _arr(C.c_float, cv), _arr(C.c_float, ch), ops._ptr(dloss), _ptrs(outs),
         _arr(C.c_int, [ld] * L), accumulate, ops._stream())
    torch.cuda.synchronize()


# ------------------------------------------------------------ 1. kernels through the ABI ----
LEVEL_LISTS = [[(1, 1), (1, 5), (5, 1), (2, 2)], [(13, 21), (40, 57), (33, 65)], [(96, 128)]]


@pytest.mark.parametrize("with_dloss", [False, True])
@pytest.mark.parametrize("alpha", [0.0, 10.0])
@pytest.mark.parametrize("levels", LEVEL_LISTS)
def test_smooth_kernels_abi(levels, alpha, with_dloss):
    """Arbitrary level sizes (directions with no pairs, single rows and columns, partial
    blocks, a level of several blocks): each level's partial slice is Sv with coefficients
    (1, 0) and Sh with (0, 1); with mixed coefficients d(flow) matches autograd of the
    reference at stride 2, at stride 4 overwriting (padding untouched) and at stride 4
    accumulating.  alpha == 0 passes img6s = NULL."""
    n, L = 2, len(levels)
    flows = [rng_tensor((n, h, w, 2), 300 + i, scale=3.0) for i, (h, w) in enumerate(levels)]
    imgs = [rng_tensor((n, h, w, 6), 400 + i) for i, (h, w) in enumerate(levels)]
    fo = [f64(f).requires_grad_(True) for f in flows]
    sums = [ref_level_sums(f, f64(i), alpha) for f, i in zip(fo, imgs)]
    fd = [dev(f) for f in flows]
    idv = [dev(i) for i in imgs] if alpha != 0 else None
    one, zero = [1.0] * L, [0.0] * L
    for which, (cv, ch) in enumerate(((one, zero), (zero, one))):
        got = _fwd(fd, idv, n, levels, alpha, cv, ch)
        for l, (h, w) in enumerate(levels):
            want = sums[l][which].item()
            print("level", (h, w), "SvSh"[2 * which:2 * which + 2], got[l], want)
            if (h if which == 0 else w) == 1:
                assert got[l] == 0.0 and want == 0.0          # a direction with no pairs
            else:
                assert _rel(got[l], want) < REL_TOL
    cv = [0.3 + 0.1 * l for l in range(L)]
    ch = [0.7 - 0.05 * l for l in range(L)]
    g = 1.75 if with_dloss else 1.0
    (sum(a * sv + b * sh for a, b, (sv, sh) in zip(cv, ch, sums)) * g).backward()
    dloss = torch.tensor([g], device="cuda") if with_dloss else None
    # stride 2, overwrite (prefilled with NaN: every element is written)
    d2 = [torch.full((n, h, w, 2), float("nan"), device="cuda") for h, w in levels]
    _bwd(fd, idv, n, levels, alpha, cv, ch, dloss, d2, 2, 0)
    # stride 4, overwrite into buffers prefilled with 7.0
    d4 = [torch.full((n, h, w, 4), 7.0, device="cuda") for h, w in levels]
    _bwd(fd, idv, n, levels, alpha, cv, ch, dloss, d4, 4, 0)
    # stride 4, accumulate onto 7.0
    a4 = [torch.full((n, h, w, 4), 7.0, device="cuda") for h, w in levels]
    _bwd(fd, idv, n, levels, alpha, cv, ch, dloss, a4, 4, 1)
    for l, (h, w) in enumerate(levels):
        want = fo[l].grad
        e2, e4 = rel_l2(d2[l], want), rel_l2(d4[l][..., :2], want)
        ea = rel_l2(a4[l][..., :2], want + 7.0)
        print("level", (h, w), "d(flow) rel_l2: ld2 %.2e ld4 %.2e accumulate %.2e" % (e2, e4, ea))
        assert e2 < REL_TOL and e4 < REL_TOL and ea < REL_TOL
        assert torch.equal(d2[l], d4[l][..., :2])
        # the accumulating form adds the same fp32 gradient to what was there
        assert torch.equal(a4[l][..., :2], d4[l][..., :2] + 7.0)
        assert (d4[l][..., 2:] == 7.0).all() and (a4[l][..., 2:] == 7.0).all()
        if (h, w) == (1, 1):
            assert (d2[l] == 0).all() and (want == 0).all()


# ------------------------------------------------- 2. no leak across rows or batches ----
def test_smooth_no_leak_across_rows_or_images():
    """A flow constant within each image and different between the two: every difference
    the definition has is 0, so each level sum is count * sqrt(eps) and the gradient is
    exactly zero; a difference taken across a row end or an image boundary would show."""
    n, h, w = 2, 5, 7
    f = torch.empty(n, h, w, 2)
    f[0] = torch.tensor([3.0, -2.0])
    f[1] = torch.tensor([-40.0, 25.0])
    fd = [dev(f)]
    sv = _fwd(fd, None, n, [(h, w)], 0.0, [1.0], [0.0])[0]
    sh = _fwd(fd, None, n, [(h, w)], 0.0, [0.0], [1.0])[0]
    assert _rel(sv, n * (h - 1) * w * 2 * EPS ** 0.5) < REL_TOL
    assert _rel(sh, n * h * (w - 1) * 2 * EPS ** 0.5) < REL_TOL
    d = [torch.full((n, h, w, 2), float("nan"), device="cuda")]
    _bwd(fd, None, n, [(h, w)], 0.0, [0.6], [0.4], None, d, 2, 0)
    assert (d[0] == 0).all()


# ----------------------------------------------- 3./4. ops.flow_smoothness, LossLayer ----
SIZES = [(2, 64, 96), (1, 48, 80), (3, 80, 112)]


def _pyramid_case(size):
    from optical_flow_amd.data import synthetic_batch
    n, H, W = size
    batch = torch.from_numpy(synthetic_batch(n, H, W, seed=5))
    flows = [rng_tensor((n, H >> (s + 1), W >> (s + 1), 2), 50 + s, scale=2.0) for s in range(4)]
    return batch, flows


@pytest.mark.parametrize("alpha", [0.0, 10.0])
@pytest.mark.parametrize("size", SIZES)
def test_flow_smoothness_op(size, alpha):
    """ops.flow_smoothness: the value and all four d(flow) (odd level sizes at (1, 48, 80)
    and (3, 80, 112))."""
    from optical_flow_amd import ops
    batch, flows = _pyramid_case(size)
    fo = [f64(f).requires_grad_(True) for f in flows]
    so = ref_smooth(f64(batch), fo, alpha)
    so.backward()
    fd = [dev(f).requires_grad_(True) for f in flows]
    sd = ops.flow_smoothness(dev(batch), fd, edge_alpha=alpha)
    sd.backward()
    print("smooth", sd.item(), so.item(), [rel_l2(a.grad, b.grad) for a, b in zip(fd, fo)])
    assert sd.shape == () and _rel(sd.item(), so.item()) < REL_TOL
    for a, b in zip(fd, fo):
        assert rel_l2(a.grad, b.grad) < REL_TOL


@pytest.mark.parametrize("size", SIZES)
def test_loss_layer_with_smoothness(size):
    """LossLayer(smoothness_weight=0.2, edge_alpha=10): the loss and every d(flow) against
    photometric + 0.2 * smooth of the reference."""
    from optical_flow_amd.loss import LossLayer
    batch, flows = _pyramid_case(size)
    fo = [f64(f).requires_grad_(True) for f in flows]
    lo = R.photometric_loss(f64(batch), fo) + 0.2 * ref_smooth(f64(batch), fo, 10.0)
    lo.backward()
    fd = [dev(f).requires_grad_(True) for f in flows]
    ld = LossLayer(smoothness_weight=0.2, edge_alpha=10)(dev(batch), fd)
    ld.backward()
    print("loss", ld.item(), lo.item(), [rel_l2(a.grad, b.grad) for a, b in zip(fd, fo)])
    assert _rel(ld.item(), lo.item()) < REL_TOL
    for a, b in zip(fd, fo):
        assert rel_l2(a.grad, b.grad) < REL_TOL


# ------------------------------------------------------------ 5./6. through the model ----
# Net seed 0 and batch seed 1236 at 64 x 64, B = 2: the float32 oracle's step is within
# REL_TOL of its float64 step here (loss 8e-8, worst parameter gradient 5.8e-6 with four
# levels; 2e-9 and 3.6e-6 with five, flow gradients 8e-6), so the case is well conditioned.
# tests/test_gpu_bn_train.py explains what the warp's floor() kinks do to other draws: batch
# seed 7 with five levels puts the float32 oracle 3.2e-3 from float64 on one gradient.
NET_SEED, BATCH_SEED = 0, 1236


def _oracle_step(batch, vals, levels, weight, alpha, dtype=torch.float64):
    from optical_flow_amd.params import encoder_blocks
    p = {k: torch.tensor(v).to(dtype) for k, v in vals.items()}
    tr = {k: v.requires_grad_(True) for k, v in p.items()
          if not k.endswith(("moving_mean", "moving_variance"))}
    b = torch.tensor(batch).to(dtype)
    flows = R.flow_net(b, p, list(encoder_blocks(levels)))
    for f in flows:
        f.retain_grad()
    loss = R.photometric_loss(b, flows) + weight * ref_smooth(b, flows, alpha)
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
    return net, vals, batch, Trainer(net, loss_layer=LossLayer(0.2, 10))


def test_train_step_with_smoothness():
    """One Trainer.train_step with LossLayer(0.2, 10) at 64 x 64, B = 2, fp32: the flows'
    gradients travel through the FlowGrad buffers (photometric write, smoothness add, then
    upscale_flow's add).  Loss and every parameter gradient against the float64 oracle's
    flow_net + the reference loss above."""
    net, vals, batch, trainer = _model_case()
    loss_o, _, grads_o = _oracle_step(batch, vals, 4, 0.2, 10.0)
    loss, _ = trainer.train_step(dev(torch.from_numpy(batch)))
    torch.cuda.synchronize()
    grads = net.store.grads()
    assert set(grads) == set(grads_o)
    errs = sorted(((rel_l2(g, grads_o[k]), k) for k, g in grads.items()), reverse=True)
    print("loss", loss.item(), loss_o.item(), "worst gradients", errs[:4])
    assert _rel(loss.item(), loss_o.item()) < REL_TOL
    assert errs[0][0] < REL_TOL, errs[0]


def test_five_levels_with_smoothness():
    """levels=5 at 64 x 64 (five flows, the coarsest 2 x 2; six groups in the loss's final
    sum): the loss value and the flows' gradients."""
    from optical_flow_amd.loss import LossLayer
    net, vals, batch, _ = _model_case(levels=5)
    loss_o, flows_o, _ = _oracle_step(batch, vals, 5, 0.2, 10.0)
    bd = dev(torch.from_numpy(batch))
    net.store.zero_grad()
    flows = net(bd)
    assert len(flows) == 5 and flows[-1].shape == (2, 2, 2, 2)
    for f in flows:
        f.retain_grad()
    loss = LossLayer(0.2, 10)(bd, flows)
    loss.backward()
    torch.cuda.synchronize()
    errs = [rel_l2(f.grad, fo.grad) for f, fo in zip(flows, flows_o)]
    print("loss", loss.item(), loss_o.item(), "d(flow)", errs)
    assert _rel(loss.item(), loss_o.item()) < REL_TOL
    assert max(errs) < REL_TOL, errs


def test_train_step_with_smoothness_is_deterministic():
    """The step of test_train_step_with_smoothness twice from the same state: losses and all
    gradients bitwise equal (no atomics in the new kernels)."""
    res = []
    for _ in range(2):
        net, vals, batch, trainer = _model_case()
        loss, _ = trainer.train_step(dev(torch.from_numpy(batch)))
        torch.cuda.synchronize()
        res.append((loss.clone(), net.store.grad_arena.clone()))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])


def test_train_command_logs_the_settings(tmp_path):
    """python -m optical_flow_amd.train --smoothness-weight --edge-alpha --log: the JSONL
    starts with a header record holding both values, then one record per step."""
    import json
    from optical_flow_amd.train import main
    log = tmp_path / "log.jsonl"
    main(["--height", "64", "--width", "64", "--batch", "1", "--steps", "2",
          "--smoothness-weight", "0.2", "--edge-alpha", "10", "--log", str(log)])
    recs = [json.loads(l) for l in open(log).read().splitlines() if l]
    assert recs[0]["smoothness_weight"] == 0.2 and recs[0]["edge_alpha"] == 10.0
    assert "step" not in recs[0] and [r["step"] for r in recs[1:]] == [0, 1]
    assert all(r["loss"] == r["loss"] and abs(r["loss"]) < 1e3 for r in recs[1:])


# ------------------------------------------------------------------ 7. default unchanged ----
def test_default_loss_layer_is_photometric_loss():
    """LossLayer() is the reference's layer: bitwise ops.photometric_loss, value and d(flow)."""
    from optical_flow_amd import ops
    from optical_flow_amd.loss import LossLayer
    batch, flows = _pyramid_case((2, 64, 96))
    bd = dev(batch)
    out = []
    for fn in (LossLayer(), lambda b, f: ops.photometric_loss(b, f)):
        fd = [dev(f).requires_grad_(True) for f in flows]
        loss = fn(bd, fd)
        loss.backward()
        out.append((loss.detach(), [f.grad for f in fd]))
    assert torch.equal(out[0][0], out[1][0])
    for a, b in zip(out[0][1], out[1][1]):
        assert torch.equal(a, b)
