"""The second-order edge-aware flow smoothness term (DESIGN.md "Second-order smoothness";
include/oflow.h of_flow_smooth2_*_multi): the kernels through the C ABI, ops.flow_smoothness(
order=2), LossLayer(smoothness_order=2), the launch sequences and a whole train step, against a
float64 reference written here from the definition

    rho(d)       = sqrt(d^2 + eps)
    d2v[b,i,j,c] = f[b,i-1,j,c] - 2 f[b,i,j,c] + f[b,i+1,j,c]          1 <= i <= h-2
    wv2[b,i,j]   = exp(-alpha * mean_{c<3} |img[b,i-1,j,c] - img[b,i+1,j,c]|)
    Sv2          = sum wv2 * rho(d2v),  Sh2 likewise along j
    smooth2_s    = Sv2 / (B (h-2) w 2) + Sh2 / (B h (w-2) 2),  smooth2 = mean_s smooth2_s

(a direction with h < 3 / w < 3 contributes 0) with oracle.ref_flow's resize for the pyramid and
its photometric loss for the other term.  Tolerance: the project's REL_TOL (rel_l2 on gradients,
relative error on scalars)."""
import ctypes as C
import functools

import pytest
import torch

from helpers import REL_TOL, dev, f64, rel_l2, rng_tensor
from oracle import ref_flow as R

pytestmark = pytest.mark.gpu

EPS = 1e-4


# ---------------------------------------------------------------- float64 reference ----
def ref_level_sums2(f, img, alpha, eps=EPS):
    """(Sv2, Sh2) of one level; img may be None when alpha == 0.  A direction shorter than 3
    has empty slices and sums to 0."""
    dv = f[:, :-2] - 2 * f[:, 1:-1] + f[:, 2:]
    dh = f[:, :, :-2] - 2 * f[:, :, 1:-1] + f[:, :, 2:]
    rv = torch.sqrt(dv * dv + eps)
    rh = torch.sqrt(dh * dh + eps)
    if alpha != 0:
        i1 = img[..., :3]
        rv = rv * torch.exp(-alpha * (i1[:, :-2] - i1[:, 2:]).abs().mean(-1, keepdim=True))
        rh = rh * torch.exp(-alpha * (i1[:, :, :-2] - i1[:, :, 2:]).abs().mean(-1, keepdim=True))
    return rv.sum(), rh.sum()


def ref_smooth2(batch, flows, alpha, eps=EPS):
    H, W = batch.shape[1], batch.shape[2]
    total = batch.new_zeros(())
    for s, f in enumerate(flows):
        n, h, w, _ = f.shape
        img = None
        if alpha != 0:
            assert h == int(H / 2.0 ** (s + 1)) and w == int(W / 2.0 ** (s + 1))
            img = R.resize_bilinear(batch, h, w)
        sv, sh = ref_level_sums2(f, img, alpha, eps)
        if h > 2:
            total = total + sv / (n * (h - 2) * w * 2)
        if w > 2:
            total = total + sh / (n * h * (w - 2) * 2)
    return total / len(flows)


def _rel(a, b):
    return abs(a - b) / abs(b)


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def _ptrs(ts):
    return _arr(C.c_void_p, [t.data_ptr() for t in ts])


def _fwd(flows, imgs, n, levels, alpha, cv, ch, eps=EPS, entry="of_flow_smooth2"):
    """<entry>_fwd_multi -> per-level partial-slice sums (float64, on the host)."""
    from optical_flow_amd import _lib, ops
    from optical_flow_amd._lib import call
    L = len(levels)
    nparts = [getattr(_lib.lib(), entry + "_partials")(n, h, w) for h, w in levels]
    parts = torch.full((sum(nparts),), float("nan"), device="cuda")
    call(entry + "_fwd_multi", _ptrs(imgs) if imgs is not None else None, _ptrs(flows), n,
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
    call("of_flow_smooth2_bwd_multi", _ptrs(imgs) if imgs is not None else None, _ptrs(flows),
         n, _arr(C.c_int, [h for h, _ in levels]), _arr(C.c_int, [w for _, w in levels]), L,
         alpha, eps, _arr(C.c_float, cv), _arr(C.c_float, ch), ops._ptr(dloss), _ptrs(outs),
         _arr(C.c_int, [ld] * L), accumulate, ops._stream())
    torch.cuda.synchronize()


# ------------------------------------------------------------ 1. kernels through the ABI ----
# directions with no triple and a single triple; an exact 8 x 32 tile, one row / column over,
# triples and gathers that straddle tile boundaries both ways; several ragged tiles per image
LEVEL_LISTS = [[(1, 1), (2, 5), (5, 2), (3, 3)], [(8, 32), (9, 33), (17, 70)],
               [(40, 57), (33, 65)]]


@pytest.mark.parametrize("with_dloss", [False, True])
@pytest.mark.parametrize("alpha", [0.0, 10.0])
@pytest.mark.parametrize("levels", LEVEL_LISTS)
def test_smooth2_kernels_abi(levels, alpha, with_dloss):
    """Each level's partial slice is Sv2 with coefficients (1, 0) and Sh2 with (0, 1); with
    mixed coefficients d(flow) matches autograd of the reference at stride 2, at stride 4
    overwriting (padding untouched) and at stride 4 accumulating.  alpha == 0 passes
    img6s = NULL."""
    n, L = 2, len(levels)
    flows = [rng_tensor((n, h, w, 2), 300 + i, scale=3.0) for i, (h, w) in enumerate(levels)]
    imgs = [rng_tensor((n, h, w, 6), 400 + i) for i, (h, w) in enumerate(levels)]
    fo = [f64(f).requires_grad_(True) for f in flows]
    sums = [ref_level_sums2(f, f64(i), alpha) for f, i in zip(fo, imgs)]
    fd = [dev(f) for f in flows]
    idv = [dev(i) for i in imgs] if alpha != 0 else None
    one, zero = [1.0] * L, [0.0] * L
    for which, (cv, ch) in enumerate(((one, zero), (zero, one))):
        got = _fwd(fd, idv, n, levels, alpha, cv, ch)
        for l, (h, w) in enumerate(levels):
            want = sums[l][which].item()
            print("level", (h, w), ("Sv2", "Sh2")[which], got[l], want)
            if (h if which == 0 else w) < 3:
                assert got[l] == 0.0 and want == 0.0          # a direction with no triple
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
        assert not torch.isnan(d2[l]).any()
        assert e2 < REL_TOL and e4 < REL_TOL and ea < REL_TOL
        assert torch.equal(d2[l], d4[l][..., :2])
        # the accumulating form adds the same fp32 gradient to what was there
        assert torch.equal(a4[l][..., :2], d4[l][..., :2] + 7.0)
        assert (d4[l][..., 2:] == 7.0).all() and (a4[l][..., 2:] == 7.0).all()
        if h < 3 and w < 3:
            assert (d2[l] == 0).all() and (want == 0).all()
        if h < 3:       # no vertical triple: the gradient is the horizontal term's alone
            got_h = [torch.full((n, hh, ww, 2), float("nan"), device="cuda") for hh, ww in levels]
            _bwd(fd, idv, n, levels, alpha, zero, ch, dloss, got_h, 2, 0)
            assert torch.equal(got_h[l], d2[l])


# ------------------------------------------------- 2. no leak across rows or images ----
@pytest.mark.parametrize("alpha", [0.0, 10.0])
def test_smooth2_affine_flow_costs_nothing(alpha):
    """A flow affine in (i, j) with small integer coefficients, different in the two images, on
    a level of more than one tile: every second difference the definition has is exactly 0, so
    Sv2 = sqrt(eps) * sum of the weights (n (h-2) w 2 sqrt(eps) without them), Sh2 likewise,
    and the gradient is exactly zero.  A triple taken across a row end, across an image
    boundary or from a stale halo would show.  The first-order term charges the same flow at
    every pair: its sums are nowhere near count * sqrt(eps)."""
    n, h, w = 2, 11, 37
    i = torch.arange(h, dtype=torch.float32).view(h, 1)
    j = torch.arange(w, dtype=torch.float32).view(1, w)
    f = torch.empty(n, h, w, 2)
    f[0, ..., 0], f[0, ..., 1] = 2 * i - 3 * j + 5, -1 * i + 2 * j - 7
    f[1, ..., 0], f[1, ..., 1] = -4 * i + 1 * j + 40, 3 * i + 3 * j - 25
    img = rng_tensor((n, h, w, 6), 77)
    fd = [dev(f)]
    idv = [dev(img)] if alpha != 0 else None
    sv = _fwd(fd, idv, n, [(h, w)], alpha, [1.0], [0.0])[0]
    sh = _fwd(fd, idv, n, [(h, w)], alpha, [0.0], [1.0])[0]
    want_v, want_h = (s.item() for s in ref_level_sums2(f64(f), f64(img), alpha))
    print("Sv2", sv, want_v, "Sh2", sh, want_h)
    if alpha == 0:
        assert _rel(want_v, n * (h - 2) * w * 2 * EPS ** 0.5) < 1e-12
        assert _rel(want_h, n * h * (w - 2) * 2 * EPS ** 0.5) < 1e-12
    assert _rel(sv, want_v) < REL_TOL and _rel(sh, want_h) < REL_TOL
    d = [torch.full((n, h, w, 2), float("nan"), device="cuda")]
    _bwd(fd, idv, n, [(h, w)], alpha, [0.6], [0.4], None, d, 2, 0)
    assert (d[0] == 0).all()
    # the orders differ: the first-order entry on the same flow
    sv1 = _fwd(fd, idv, n, [(h, w)], 0.0, [1.0], [0.0], entry="of_flow_smooth")[0]
    sh1 = _fwd(fd, idv, n, [(h, w)], 0.0, [0.0], [1.0], entry="of_flow_smooth")[0]
    assert sv1 > 10 * n * (h - 1) * w * 2 * EPS ** 0.5
    assert sh1 > 10 * n * h * (w - 1) * 2 * EPS ** 0.5


# ----------------------------------------------- 3. ops.flow_smoothness, LossLayer ----
SIZES = [(2, 64, 96), (1, 48, 80), (3, 80, 112)]


@functools.lru_cache(maxsize=None)
def _pyramid_case(size):
    from optical_flow_amd.data import synthetic_batch
    n, H, W = size
    batch = torch.from_numpy(synthetic_batch(n, H, W, seed=5))
    flows = [rng_tensor((n, H >> (s + 1), W >> (s + 1), 2), 50 + s, scale=2.0) for s in range(4)]
    return batch, flows


@pytest.mark.parametrize("alpha", [0.0, 10.0])
@pytest.mark.parametrize("size", SIZES)
def test_flow_smoothness_order2_op(size, alpha):
    """ops.flow_smoothness(order=2): the value and all four d(flow)."""
    from optical_flow_amd import ops
    batch, flows = _pyramid_case(size)
    fo = [f64(f).requires_grad_(True) for f in flows]
    so = ref_smooth2(f64(batch), fo, alpha)
    so.backward()
    fd = [dev(f).requires_grad_(True) for f in flows]
    sd = ops.flow_smoothness(dev(batch), fd, edge_alpha=alpha, order=2)
    sd.backward()
    print("smooth2", sd.item(), so.item(), [rel_l2(a.grad, b.grad) for a, b in zip(fd, fo)])
    assert sd.shape == () and _rel(sd.item(), so.item()) < REL_TOL
    for a, b in zip(fd, fo):
        assert rel_l2(a.grad, b.grad) < REL_TOL


@pytest.mark.parametrize("size", SIZES)
def test_loss_layer_order2(size):
    """LossLayer(0.2, 10, smoothness_order=2): the loss and every d(flow) against photometric +
    0.2 * smooth2 of the reference."""
    from optical_flow_amd.loss import LossLayer
    batch, flows = _pyramid_case(size)
    fo = [f64(f).requires_grad_(True) for f in flows]
    lo = R.photometric_loss(f64(batch), fo) + 0.2 * ref_smooth2(f64(batch), fo, 10.0)
    lo.backward()
    fd = [dev(f).requires_grad_(True) for f in flows]
    ld = LossLayer(0.2, 10, smoothness_order=2)(dev(batch), fd)
    ld.backward()
    print("loss", ld.item(), lo.item(), [rel_l2(a.grad, b.grad) for a, b in zip(fd, fo)])
    assert _rel(ld.item(), lo.item()) < REL_TOL
    for a, b in zip(fd, fo):
        assert rel_l2(a.grad, b.grad) < REL_TOL


def test_loss_layer_order1_is_the_default_layer():
    """LossLayer(0.2, 10, smoothness_order=1) is LossLayer(0.2, 10): bitwise, loss and d(flow)."""
    from optical_flow_amd.loss import LossLayer
    batch, flows = _pyramid_case(SIZES[0])
    bd = dev(batch)
    out = []
    for layer in (LossLayer(0.2, 10, smoothness_order=1), LossLayer(0.2, 10)):
        fd = [dev(f).requires_grad_(True) for f in flows]
        loss = layer(bd, fd)
        loss.backward()
        out.append((loss.detach(), [f.grad for f in fd]))
    assert torch.equal(out[0][0], out[1][0])
    for a, b in zip(out[0][1], out[1][1]):
        assert torch.equal(a, b)


# ------------------------------------------------- 4. launch sequences and FlowGrads ----
PYR, SUM = "of_pyramid6", "of_sum_partials"
PF, PB = "of_photo_l1_fwd_multi", "of_photo_l1_bwd_multi"
CF, CB = "of_census_fwd_multi", "of_census_bwd_multi"
S1F, S1B = "of_flow_smooth_fwd_multi", "of_flow_smooth_bwd_multi"
S2F, S2B = "of_flow_smooth2_fwd_multi", "of_flow_smooth2_bwd_multi"


def _three2(ops, b, f):
    return ops.census_flow_loss(b, f, 0.5, 3, 0.5, 0.2, 10, smoothness_order=2)


# id: (call, forward names, backward names)
ROWS = {
    "flow_loss_order2": (lambda ops, b, f: ops.flow_loss(b, f, 0.2, 10, smoothness_order=2),
                         [PYR, PF, S2F, SUM], [PB, S2B + "(acc 1)"]),
    "smoothness2_alpha0": (lambda ops, b, f: ops.flow_smoothness(b, f, edge_alpha=0, order=2),
                           [S2F, SUM], [S2B + "(acc 0)"]),
    "smoothness2_alpha10": (lambda ops, b, f: ops.flow_smoothness(b, f, edge_alpha=10, order=2),
                            [PYR, S2F, SUM], [S2B + "(acc 0)"]),
    "three_terms_order2": (_three2, [PYR, PF, CF, S2F, SUM],
                           [PB, CB + "(acc 1)", S2B + "(acc 1)"]),
    "flow_loss_order1": (lambda ops, b, f: ops.flow_loss(b, f, 0.2, 10, smoothness_order=1),
                         [PYR, PF, S1F, SUM], [PB, S1B + "(acc 1)"]),
    "smoothness_order1": (lambda ops, b, f: ops.flow_smoothness(b, f, edge_alpha=0, order=1),
                          [S1F, SUM], [S1B + "(acc 0)"]),
    "flow_loss_default": (lambda ops, b, f: ops.flow_loss(b, f, 0.2, 10),
                          [PYR, PF, S1F, SUM], [PB, S1B + "(acc 1)"]),
}


@functools.lru_cache(maxsize=None)
def _small_inputs():
    """n = 2, a 32 x 32 batch and four flows of 16 x 16 down to 2 x 2 (no triple at all)."""
    from optical_flow_amd.data import synthetic_batch
    batch = dev(torch.from_numpy(synthetic_batch(2, 32, 32, seed=5)))
    flows = [rng_tensor((2, 32 >> (s + 1), 32 >> (s + 1), 2), 50 + s, scale=2.0)
             for s in range(4)]
    return batch, flows


def _spy(monkeypatch, ops):
    called = []
    real = ops.call

    def call(name, *a):
        # accumulate is the argument before the stream
        called.append("%s(acc %d)" % (name, a[-2]) if name in (CB, S1B, S2B) else name)
        return real(name, *a)
    monkeypatch.setattr(ops, "call", call)
    return called


@pytest.mark.parametrize("row", list(ROWS))
def test_launch_sequence(monkeypatch, row):
    """One forward and one backward: the entry names in order, and the accumulate flag."""
    from optical_flow_amd import ops
    fn, fwd, bwd = ROWS[row]
    batch, flows = _small_inputs()
    fd = [dev(f).requires_grad_(True) for f in flows]
    called = _spy(monkeypatch, ops)
    loss = fn(ops, batch, fd)
    assert called == fwd
    loss.backward()
    torch.cuda.synchronize()
    assert called == fwd + bwd
    if "order2" not in row and "smoothness2" not in row:
        assert not any("smooth2" in c for c in called)


def _grads(fn, ops, batch, flows, attach):
    fd = [dev(f).requires_grad_(True) for f in flows]
    fgs = []
    if attach:
        for f in fd:
            f._of_flowgrad = ops.FlowGrad(f.shape, f.device)
            fgs.append(f._of_flowgrad)
    fn(ops, batch, fd).backward()
    torch.cuda.synchronize()
    return [f.grad for f in fd], fgs


def test_three_term_order2_loss_fills_the_flowgrads():
    """With FlowGrads attached the three-term order-2 loss writes them: filled, bitwise the
    plain gradient, channels 2-3 exactly 0."""
    from optical_flow_amd import ops
    batch, flows = _small_inputs()
    plain, _ = _grads(_three2, ops, batch, flows, False)
    routed, fgs = _grads(_three2, ops, batch, flows, True)
    try:
        for g, p, fg in zip(routed, plain, fgs):
            assert fg.filled
            assert torch.equal(g, p)
            assert torch.equal(fg.buffer()[..., :2], p)
            assert (fg.buffer()[..., 2:] == 0).all()
    finally:
        for fg in fgs:
            fg.release()


def test_standalone_order2_term_leaves_the_flowgrads_alone():
    from optical_flow_amd import ops
    fn = ROWS["smoothness2_alpha10"][0]
    batch, flows = _small_inputs()
    plain, _ = _grads(fn, ops, batch, flows, False)
    routed, fgs = _grads(fn, ops, batch, flows, True)
    try:
        for g, p, fg in zip(routed, plain, fgs):
            assert not fg.filled
            assert g.shape == p.shape and g.is_contiguous()
            assert torch.equal(g, p)
    finally:
        for fg in fgs:
            fg.release()


# ------------------------------------------------------------ 5. through the model ----
# Net seed 0 and batch seed 1236 at 64 x 64, B = 2 (the first-order test's case): with the
# order-2 loss the float32 oracle's step (_oracle_step(dtype=torch.float32), on the CPU) is
# within REL_TOL of its float64 step: loss 7.2e-8, worst parameter gradient 7.4e-6 with four
# levels; 4.7e-8 and 6.5e-6 with five, flow gradients 1.4e-5 at most.  So the case is well
# conditioned (tests/test_gpu_smooth_loss.py explains what the warp's floor() kinks do to
# other draws).
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
    loss = R.photometric_loss(b, flows) + weight * ref_smooth2(b, flows, alpha)
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
    return net, vals, batch, Trainer(net, loss_layer=LossLayer(0.2, 10, smoothness_order=2))


def test_train_step_order2():
    """One Trainer.train_step with LossLayer(0.2, 10, smoothness_order=2) at 64 x 64, B = 2,
    fp32: loss and every parameter gradient against the float64 oracle's flow_net + the
    reference loss above."""
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


def test_five_levels_order2():
    """levels=5 at 64 x 64: the coarsest flow is 2 x 2, which has no triple in either
    direction.  The loss value and the flows' gradients at all five levels."""
    from optical_flow_amd.loss import LossLayer
    net, vals, batch, _ = _model_case(levels=5)
    loss_o, flows_o, _ = _oracle_step(batch, vals, 5, 0.2, 10.0)
    bd = dev(torch.from_numpy(batch))
    net.store.zero_grad()
    flows = net(bd)
    assert len(flows) == 5 and flows[-1].shape == (2, 2, 2, 2)
    for f in flows:
        f.retain_grad()
    loss = LossLayer(0.2, 10, smoothness_order=2)(bd, flows)
    loss.backward()
    torch.cuda.synchronize()
    errs = [rel_l2(f.grad, fo.grad) for f, fo in zip(flows, flows_o)]
    print("loss", loss.item(), loss_o.item(), "d(flow)", errs)
    assert _rel(loss.item(), loss_o.item()) < REL_TOL
    assert max(errs) < REL_TOL, errs


def test_train_step_order2_is_deterministic():
    """The step of test_train_step_order2 twice from the same state: losses and the gradient
    arena bitwise equal (no atomics in the new kernels)."""
    res = []
    for _ in range(2):
        net, vals, batch, trainer = _model_case()
        loss, _ = trainer.train_step(dev(torch.from_numpy(batch)))
        torch.cuda.synchronize()
        res.append((loss.clone(), net.store.grad_arena.clone()))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])


def test_train_command_order2(tmp_path):
    """python -m optical_flow_amd.train --smoothness-order 2 --log: the header record holds the
    order, then one finite record per step."""
    import json
    from optical_flow_amd.train import main
    log = tmp_path / "log.jsonl"
    main(["--height", "64", "--width", "64", "--batch", "1", "--steps", "2",
          "--smoothness-weight", "0.2", "--edge-alpha", "10", "--smoothness-order", "2",
          "--log", str(log)])
    recs = [json.loads(l) for l in open(log).read().splitlines() if l]
    assert recs[0]["smoothness_order"] == 2
    assert recs[0]["smoothness_weight"] == 0.2 and recs[0]["edge_alpha"] == 10.0
    assert "step" not in recs[0] and [r["step"] for r in recs[1:]] == [0, 1]
    assert all(r["loss"] == r["loss"] and abs(r["loss"]) < 1e3 for r in recs[1:])
