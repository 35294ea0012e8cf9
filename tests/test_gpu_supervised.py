"""The supervised loss term on the GPU (supervised_loss.hip, ops.supervised_flow_loss,
LossLayer(supervised_weight=...), Trainer.train_step(..., gt=...)) against the float64
restatement of tests/supervised_ref.py.  Tolerance: helpers.REL_TOL, relative error on scalars,
rel_l2 on gradients; tests/test_supervised_host.py shows an fp32 evaluation of the restatement
to be within REL_TOL / 10 on every input used here.

Twenty eager steps on one labelled batch (test_twenty_steps_descend) bring the supervised loss
from its first step's value down; DESIGN.md "Supervised term" records both.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import kitti_flow_np as K
import supervised_ref as R
from helpers import REL_TOL, dev, rel_l2

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return abs(a - b) / (abs(b) if b else 1.0)


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_abi(flows, maps, q, eps, coefs, raw=None, descs=None):
    """of_supervised_fwd_multi on NaN-prefilled outputs: ([per-level partial sums], [planes],
    the partials)."""
    from optical_flow_amd._lib import call, lib
    from optical_flow_amd.gt_raw import pack_gt_raw
    fl = [dev(_t(f)) for f in flows]
    n, L = fl[0].shape[0], len(fl)
    if raw is None:
        raw, descs = pack_gt_raw(maps)
    draw = dev(_t(raw))
    mh, mw = int(descs["h"].max()), int(descs["w"].max())
    hs, ws = [f.shape[1] for f in fl], [f.shape[2] for f in fl]
    nparts = [lib().of_supervised_partials(n, h, w, mh, mw) for h, w in zip(hs, ws)]
    parts = torch.full((sum(nparts),), float("nan"), device="cuda")
    planes = [torch.full_like(f, float("nan")) for f in fl]
    wsb = lib().of_supervised_workspace_bytes(n, mh, mw)
    wsp = torch.empty(wsb // 4 + 4, device="cuda")
    arr = lambda ct, v: (ct * len(v))(*v)
    call("of_supervised_fwd_multi", arr(C.c_void_p, [f.data_ptr() for f in fl]), n, len(descs),
         arr(C.c_int, hs), arr(C.c_int, ws), L, C.c_void_p(draw.data_ptr()),
         descs.ctypes.data_as(C.c_void_p), draw.numel(), mh, mw, q, eps, arr(C.c_float, coefs),
         C.c_void_p(wsp.data_ptr()), wsb, arr(C.c_void_p, [p.data_ptr() for p in planes]),
         C.c_void_p(parts.data_ptr()), _stream())
    torch.cuda.synchronize()
    sums, off = [], 0
    for k in nparts:
        sums.append(parts[off:off + k].double().sum().item())
        off += k
    return sums, planes, parts


def check_case(flows, maps, q, ref, what, eps=R.EPS):
    """One ABI call over all levels with coefficients 1 / L against the restatement ``ref``;
    every output written; two runs bitwise equal."""
    L = len(flows)
    _, s_ref, g_ref = ref
    sums, planes, parts = run_abi(flows, maps, q, eps, [1.0 / L] * L)
    assert bool(torch.isfinite(parts).all())
    for l in range(L):
        assert bool(torch.isfinite(planes[l]).all()), "level %d: plane not fully written" % l
        ev, eg = _rel(sums[l], s_ref[l] / L), rel_l2(planes[l], _t(g_ref[l]))
        print("%s q=%g level %d: value %.7g / %.7g (rel %.2e), gradient rel_l2 %.2e"
              % (what, q, l, sums[l], s_ref[l] / L, ev, eg))
        assert ev <= REL_TOL and eg <= REL_TOL
    sums2, planes2, parts2 = run_abi(flows, maps, q, eps, [1.0 / L] * L)
    assert torch.equal(parts, parts2)
    assert all(torch.equal(a, b) for a, b in zip(planes, planes2))
    return sums, planes


# ------------------------------------------------------------- 1. the kernel, all levels ----
@pytest.mark.parametrize("q", R.QS)
def test_kernel_matches_restatement(q):
    """n = 3, maps of three sizes (odd widths), four levels in one call."""
    flows, maps = R.case("three_sizes")
    check_case(flows, maps, q, R.reference("three_sizes", q), "three_sizes")


@pytest.mark.parametrize("shift", [2, 1], ids=["plus2", "odd"])
def test_maps_at_unaligned_offsets(shift):
    """A map whose offset is not 16-byte aligned (counting pass) or odd (forward) is read byte
    by byte: bitwise the same results."""
    from optical_flow_amd.gt_raw import DESC_DTYPE
    flows, maps = R.case("three_sizes")
    n, L = len(maps), len(flows)
    desc = np.zeros(n, DESC_DTYPE)
    total = 256
    for i, m in enumerate(maps):
        desc[i] = (total + shift, m.shape[0], m.shape[1])
        total += -(-(m.nbytes + shift) // 256) * 256
    raw = np.zeros(total, np.uint8)
    raw[:16 * n] = desc.view(np.uint8)
    for d, m in zip(desc, maps):
        raw[d["offset"]:d["offset"] + m.nbytes] = m.reshape(-1).view(np.uint8)
    _, planes, parts = run_abi(flows, maps, 0.4, R.EPS, [1.0 / L] * L)
    _, planes_s, parts_s = run_abi(flows, maps, 0.4, R.EPS, [1.0 / L] * L, raw, desc)
    assert torch.equal(parts, parts_s)
    assert all(torch.equal(a, b) for a, b in zip(planes, planes_s))


# ------------------------------------------------------------------------ 2. edge shapes ----
@pytest.mark.parametrize("name", ["one_cell_grid", "one_pixel_map", "wide", "coarse_under_full"])
@pytest.mark.parametrize("q", R.QS)
def test_edge_shapes(name, q):
    """A 1 x 1 grid under a 5 x 7 map (every clamp active), a 1 x 1 map, one more shape with
    several blocks, and a 3 x 5 grid under a full-size map (> 10^5 pixels per cell)."""
    flows, maps = R.case(name)
    check_case(flows, maps, q, R.reference(name, q), name)


def test_one_empty_image():
    """An image without a valid pixel: its plane is exactly 0 and the others are normalised by
    the non-empty count."""
    flows, maps = R.case("three_sizes")
    maps = [maps[0], np.zeros_like(maps[1]), maps[2]]
    ref = R.supervised_ref(flows, maps, 1.0, R.EPS)
    _, planes = check_case(flows, maps, 1.0, ref, "one empty")
    for p in planes:
        assert not bool(p[1].any()) and bool(p[0].any()) and bool(p[2].any())


def test_every_image_empty():
    flows, maps = R.case("three_sizes")
    maps = [np.zeros_like(m) for m in maps]
    sums, planes, parts = run_abi(flows, maps, 0.4, R.EPS, [0.25] * 4)
    assert not bool(parts.any()) and all(not bool(p.any()) for p in planes)
    assert sums == [0.0] * 4


# --------------------------------------------------------------------- 3. known answers ----
def _const_case(offset):
    flow = np.full((2, 2, 4, 2), 0.5, np.float32)           # (u, v) = (0.5 * 8/4, 0.5 * 6/2)
    rgb = np.ones((6, 8, 3), np.uint16)
    rgb[:, :, 0] = 32768 + 64 * (1 + offset[0])
    rgb[:, :, 1] = 32768 + 96 + 64 * offset[1]
    return [flow], [rgb, rgb.copy()]


@pytest.mark.parametrize("q", R.QS)
def test_constant_flow_known_answers(q):
    eps = 0.01
    flows, maps = _const_case((0, 0))
    sums, planes, _ = run_abi(flows, maps, q, eps, [1.0])
    assert _rel(sums[0], eps ** q) <= REL_TOL
    assert not bool(planes[0].any())                        # e = 0 exactly: no gradient
    flows, maps = _const_case((3, 4))
    sums, planes, _ = run_abi(flows, maps, q, eps, [1.0])
    assert _rel(sums[0], (25.0 + eps * eps) ** (q / 2)) <= REL_TOL
    assert bool(torch.isfinite(planes[0]).all()) and bool(planes[0].any())


def test_value_is_the_evaluators_epe():
    """q = 1, eps = 1e-6, one level: the mean end-point error evaluate.flow_metrics gives."""
    from optical_flow_amd.evaluate import flow_metrics
    from test_gpu_flow_eval import TOL
    flows, maps = R.case("three_sizes")
    sums, _, _ = run_abi(flows[:1], maps, 1.0, 1e-6, [1.0])
    s, v, _ = flow_metrics(dev(_t(flows[0])), maps)
    epe = (s / v.double()).mean().item()
    print("supervised value %.7f, evaluator's mean EPE %.7f" % (sums[0], epe))
    assert abs(sums[0] - epe) <= TOL


# ------------------------------------------------------------------------- 4. full size ----
@pytest.mark.parametrize("q", R.QS)
def test_full_size(q):
    """Grids (96,320) ... (12,40) under two 375 x 1242 maps: footprints of 8 x 8 to 62 x 62
    pixels, cells owned by one wave and by four."""
    flows, maps = R.case("full_size")
    check_case(flows, maps, q, R.reference("full_size", q), "full_size")


# ------------------------------------------------------------- 5. the op and LossLayer ----
@functools.lru_cache(maxsize=None)
def _layer_inputs():
    from optical_flow_amd.data import synthetic_batch
    flows, maps = R.case("layer")
    return synthetic_batch(2, 64, 128, seed=77), flows, maps


def _gt_forms(maps):
    from optical_flow_amd.gt_raw import pack_gt_raw
    raw, descs = pack_gt_raw(maps)
    return {"list": maps, "host": raw, "host+descs": (raw, descs),
            "device": (dev(_t(raw)), descs)}


@pytest.mark.parametrize("q,lw", [(1.0, None), (0.4, (0.4, 0.3, 0.2, 0.1))])
def test_supervised_flow_loss_op(q, lw):
    """ops.supervised_flow_loss alone (no image batch, no pyramid), with a non-unit upstream
    gradient; the ground truth as a list, a host buffer and a device buffer: bitwise equal."""
    from optical_flow_amd import ops
    _, flows, maps = _layer_inputs()
    v_ref, _, g_ref = R.supervised_ref(flows, maps, q, 0.02, lw)
    res = {}
    for form, gt in _gt_forms(maps).items():
        fd = [dev(_t(f)).requires_grad_(True) for f in flows]
        loss = ops.supervised_flow_loss(fd, gt, q=q, eps=0.02, level_weights=lw)
        (loss * 2.5).backward()
        res[form] = (loss.detach().clone(), [f.grad.clone() for f in fd])
    loss, grads = res["list"]
    assert _rel(loss.item(), v_ref) <= REL_TOL
    for l, g in enumerate(grads):
        err = rel_l2(g, 2.5 * _t(g_ref[l]))
        print("op q=%g level %d: gradient rel_l2 %.2e" % (q, l, err))
        assert err <= REL_TOL
    for form, (lo, gr) in res.items():
        assert torch.equal(lo, loss), form
        assert all(torch.equal(a, b) for a, b in zip(gr, grads)), form


MIXES = {
    "alone": dict(photometric_weight=0.0),
    "mixed": dict(photometric_weight=0.5, census_weight=0.5, smoothness_weight=0.2,
                  edge_alpha=10.0, smoothness_order=2),
}


@pytest.mark.parametrize("mix", list(MIXES))
def test_loss_layer_with_supervised(mix):
    """LossLayer(supervised_weight=0.7) alone (every unsupervised data weight 0: the term
    writes d(flow)) and with photometric + census + second-order smoothness (it adds): value
    and d(flow) are the sum of the separately computed terms -- the unsupervised ones from
    the same layer without the term, the supervised one from the restatement."""
    from optical_flow_amd.loss import LossLayer
    batch, flows, maps = _layer_inputs()
    batch = dev(_t(batch))
    kw = MIXES[mix]
    v_ref, _, g_ref = R.supervised_ref(flows, maps, 0.4, R.EPS)
    v_uns, g_uns = 0.0, [torch.zeros(f.shape, dtype=torch.float64) for f in flows]
    if mix == "mixed":
        fd = [dev(_t(f)).requires_grad_(True) for f in flows]
        lu = LossLayer(warp_convention="image", **kw)(batch, fd)
        (lu * 1.5).backward()
        v_uns, g_uns = lu.item(), [f.grad.double().cpu() for f in fd]
    fd = [dev(_t(f)).requires_grad_(True) for f in flows]
    layer = LossLayer(warp_convention="image", supervised_weight=0.7, supervised_q=0.4, **kw)
    loss = layer(batch, fd, gt=maps)
    (loss * 1.5).backward()
    want = v_uns + 0.7 * v_ref
    print("%s: loss %.7g, sum of the terms %.7g" % (mix, loss.item(), want))
    assert _rel(loss.item(), want) <= REL_TOL
    for l, f in enumerate(fd):
        err = rel_l2(f.grad, g_uns[l] + 1.5 * 0.7 * _t(g_ref[l]))
        print("%s level %d: gradient rel_l2 %.2e" % (mix, l, err))
        assert err <= REL_TOL


def test_loss_layer_fb_scores_the_forward_pairs_only():
    """occlusion="fb": the doubled batch's second half has no ground truth -- its supervised
    gradient is exactly 0, and the first half's is that of the plain batch."""
    from optical_flow_amd import ops
    _, flows, maps = _layer_inputs()
    doubled = [np.concatenate([f, f[::-1]]) for f in flows]
    fd = [dev(_t(f)).requires_grad_(True) for f in doubled]
    cfg = ops._LossCfg(**ops._sup_cfg(fd, maps, 1.0, 1.0, R.EPS, None))
    ops._Loss.apply(None, cfg, *fd).backward()
    f1 = [dev(_t(f)).requires_grad_(True) for f in flows]
    ops.supervised_flow_loss(f1, maps).backward()
    for a, b in zip(fd, f1):
        assert torch.equal(a.grad[:2], b.grad) and not bool(a.grad[2:].any())


# ------------------------------------------------------------------ 6. through the net ----
H, W, NET_SEED = 64, 128, 0


def _net():
    from optical_flow_amd.model import build_flow_net
    return build_flow_net(H, W, seed=NET_SEED, levels=4, warp_convention="image")


@functools.lru_cache(maxsize=None)
def _labelled_batch():
    """A batch for the 64 x 128 net and ground truth built (R.make_gt) around the seeded net's
    own finest flow, at two native sizes."""
    from optical_flow_amd.data import synthetic_batch
    batch = synthetic_batch(2, H, W, seed=1240)
    with torch.no_grad():
        flow = _net()(dev(_t(batch)))[0].cpu().numpy()
    rng = np.random.default_rng(31)
    maps = [R.make_gt(K.upsample_np(flow[i], gh, gw), rng)
            for i, (gh, gw) in enumerate([(93, 301), (80, 257)])]
    return batch, maps


def _torch_term(flows, maps, q=1.0, eps=0.01):
    return sum(R.level_value(f, maps, q, eps) for f in flows) / len(flows)


def test_parameter_gradients_through_the_net():
    """The FlowGrad route (row stride 4, upscale_flow adding afterwards): the parameter
    gradients under LossLayer(photometric_weight=0, supervised_weight=1) against those under a
    plain-torch fp32 restatement of the term on the net's flows (ordinary autograd route)."""
    from optical_flow_amd.loss import LossLayer
    batch, maps = _labelled_batch()
    batch = dev(_t(batch))
    net = _net()
    net.store.zero_grad()
    loss = LossLayer(photometric_weight=0.0, supervised_weight=1.0,
                     warp_convention="image")(batch, net(batch), gt=maps)
    loss.backward()
    torch.cuda.synchronize()
    got = net.store.grad_arena.clone()
    net.store.zero_grad()
    loss_t = _torch_term(net(batch), maps)
    loss_t.backward()
    torch.cuda.synchronize()
    want = net.store.grad_arena.clone()
    err = rel_l2(got, want)
    print("loss %.7g / %.7g, gradient arena rel_l2 %.2e" % (loss.item(), loss_t.item(), err))
    assert bool(want.any()) and _rel(loss.item(), loss_t.item()) <= REL_TOL
    assert err <= REL_TOL


# ------------------------------------------------------------------------- 7. the step ----
def _trainer(**kw):
    from optical_flow_amd.loss import LossLayer
    from optical_flow_amd.train import Trainer
    net = _net()
    return net, Trainer(net, loss_layer=LossLayer(warp_convention="image", **kw))


def test_train_step_with_ground_truth():
    batch, maps = _labelled_batch()
    net, trainer = _trainer(photometric_weight=0.0, supervised_weight=1.0, supervised_q=0.4)
    v0 = net.store.version
    loss, flows = trainer.train_step(dev(_t(batch)), gt=maps)
    torch.cuda.synchronize()
    assert net.store.version > v0
    want = R.supervised_ref([f.cpu().numpy() for f in flows], maps, 0.4, 0.01)[0]
    print("step loss %.7g, restatement on the returned flows %.7g" % (loss.item(), want))
    assert _rel(loss.item(), want) <= REL_TOL
    with pytest.raises(ValueError, match="gt"):
        trainer.train_step(dev(_t(batch)))


def test_twenty_steps_descend():
    """Twenty eager steps on one fixed labelled batch end below the first step's loss."""
    batch, maps = _labelled_batch()
    from optical_flow_amd.gt_raw import pack_gt_raw
    raw, descs = pack_gt_raw(maps)
    gt = (dev(_t(raw)), descs)
    _, trainer = _trainer(photometric_weight=0.0, supervised_weight=1.0)
    b = dev(_t(batch))
    losses = [trainer.train_step(b, k, gt=gt)[0] for k in range(20)]
    losses = [v.item() for v in losses]
    print("supervised loss, step 1: %.6f, step 20: %.6f" % (losses[0], losses[-1]))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_graphed_step_refuses_a_supervised_layer():
    batch, _ = _labelled_batch()
    _, trainer = _trainer(supervised_weight=1.0)
    with pytest.raises(RuntimeError, match="supervised"):
        trainer.graphed(dev(_t(batch)))


def test_weight_zero_step_is_the_parent_step():
    """Two trainers built alike, one through the new keyword defaults: loss and flows bitwise
    equal, and no supervised entry is called."""
    from optical_flow_amd import ops
    batch, _ = _labelled_batch()
    b = dev(_t(batch))
    _, t1 = _trainer(smoothness_weight=0.1)
    _, t2 = _trainer(smoothness_weight=0.1, supervised_weight=0.0, supervised_q=1.0,
                     supervised_eps=0.01, supervised_level_weights=None)
    called = []
    real = ops.call
    l1, f1 = t1.train_step(b)
    ops.call = lambda name, *a: (called.append(name), real(name, *a))[1]
    try:
        l2, f2 = t2.train_step(b, 0, gt=None)
    finally:
        ops.call = real
    torch.cuda.synchronize()
    assert called and not [c for c in called if c.startswith("of_supervised")]
    assert torch.equal(l1, l2) and all(torch.equal(a, c) for a, c in zip(f1, f2))
