"""GPU parity of augmentation self-supervision: of_augment_batch bit for bit against its numpy
float32 restatement, of_flow_transform and of_flow_distill_fwd against the float64 restatement
(tests/selfsup_ref.py) on the shared seeded cases (tests/selfsup_cases.py; the host tests check
the restatement's own fp32 error and the near-kink share on the same inputs), the ops entries'
autograd, _Loss additivity and its group limit, and the Trainer's self-supervised step."""
import ctypes as C

import numpy as np
import pytest
import torch

import selfsup_cases as SC
import selfsup_ref as R
from helpers import REL_TOL, rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def lib():
    from optical_flow_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load()


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()      # (a copy: the cases are read-only)


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _rec(records):
    return _dev(np.ascontiguousarray(records).view(np.uint8).copy())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ------------------------------------------------------------------- of_augment_batch ----
@pytest.mark.parametrize("colour", [False, True], ids=["plain", "colour"])
@pytest.mark.parametrize("grid,name", SC.CASES, ids=SC.IDS)
def test_augment_batch_bit_exact(grid, name, colour):
    from optical_flow_amd._lib import call
    c = SC.case(grid, name)
    n, H, W = SC.N, c["H"], c["W"]
    recs = SC.records(name, H, W, colour)
    exp = R.augment_batch_f32(c["batch"], recs)
    batch, rec = _dev(c["batch"]), _rec(recs)
    outs = []
    for _ in range(2):
        out = _nan(n, H, W, 6)                      # every element must be written
        call("of_augment_batch", _p(batch), n, H, W, _p(rec), _p(out), _stream())
        outs.append(out.cpu().numpy())
    assert np.isfinite(outs[0]).all()
    np.testing.assert_array_equal(outs[0].view(np.uint32), exp.view(np.uint32))
    np.testing.assert_array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


def test_augment_batch_entry():
    """ops.augment_batch takes the records as an AUGMENT_DTYPE array or as a CUDA uint8 tensor."""
    from optical_flow_amd import ops
    c = SC.case((12, 20), "zoom")
    exp = R.augment_batch_f32(c["batch"], c["records"])
    batch = _dev(c["batch"])
    a = ops.augment_batch(batch, c["records"])
    b = ops.augment_batch(batch, _rec(c["records"]))
    np.testing.assert_array_equal(a.cpu().numpy().view(np.uint32), exp.view(np.uint32))
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="records"):
        ops.augment_batch(batch, c["records"][:1])
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.augment_batch(batch.cpu(), c["records"])


# ------------------------------------------------------------------ of_flow_transform ----
@pytest.mark.parametrize("masked", [False, True], ids=["ones", "mask"])
@pytest.mark.parametrize("grid,name", SC.CASES, ids=SC.IDS)
def test_flow_transform(grid, name, masked):
    """The target within REL_TOL (rel_l2) of the float64 restatement; the weight equal to it
    outside the near-kink cells (at most 1 % of the cells beyond the border cells of the two
    lattice records: tests/test_selfsup_host.py), within REL_TOL of it under a teacher mask."""
    from optical_flow_amd import ops
    c = SC.case(grid, name)
    (fh, fw), n = grid, SC.N
    teacher = _dev(c["teacher"])
    mask = _dev(c["mask"]) if masked else None
    from optical_flow_amd._lib import call
    rec = _rec(c["records"])
    res = []
    for _ in range(2):
        target, weight = _nan(n, fh, fw, 2), _nan(n, fh, fw)
        call("of_flow_transform", _p(teacher), n, fh, fw, c["H"], c["W"], _p(rec), _p(mask),
             _p(target), _p(weight), _stream())
        res.append((target.cpu().numpy(), weight.cpu().numpy()))
    (target, weight), (target2, weight2) = res
    assert np.isfinite(target).all() and np.isfinite(weight).all()
    np.testing.assert_array_equal(target.view(np.uint32), target2.view(np.uint32))
    np.testing.assert_array_equal(weight.view(np.uint32), weight2.view(np.uint32))
    err = rel_l2(torch.from_numpy(target), torch.from_numpy(np.array(c["target"])))
    print("target rel_l2 %.2e" % err)
    assert err < REL_TOL
    ok = ~(c["inside_kink"] | c["visible_kink"])
    wref = c["weight_m"] if masked else c["weight"]
    if masked:
        den = np.abs(wref[ok]).max() if ok.any() else 0.0
        werr = np.abs(weight - wref)[ok].max() / (den if den > 0 else 1.0)
        print("weight rel %.2e" % werr)
        assert werr < REL_TOL
    else:
        np.testing.assert_array_equal(weight[ok], wref[ok].astype(np.float32))
    # the ops entry is this call
    t3, w3 = ops.transform_flow(teacher, c["records"], (c["H"], c["W"]), mask)
    assert torch.equal(t3.cpu(), torch.from_numpy(target))
    assert torch.equal(w3.cpu(), torch.from_numpy(weight))


# ---------------------------------------------------------------- of_flow_distill_fwd ----
@pytest.mark.parametrize("q", [1.0, 0.4])
@pytest.mark.parametrize("grid,name", SC.CASES, ids=SC.IDS)
def test_flow_distill(lib, grid, name, q):
    from optical_flow_amd._lib import call
    c = SC.case(grid, name)
    (fh, fw), n = grid, SC.N
    eps, coef = 0.01, 0.37 / (n * fh * fw)
    S, g = R.distill(c["student"], c["dtarget"], c["dweight"], q, eps)
    student, target, weight = _dev(c["student"]), _dev(c["dtarget"]), _dev(c["dweight"])
    npart = lib.of_flow_distill_partials(n, fh, fw)
    assert npart == (n * fh * fw + 1023) // 1024
    res = []
    for with_plane in (True, True, False):
        parts = _nan(npart)
        plane = _nan(n, fh, fw, 2) if with_plane else None
        call("of_flow_distill_fwd", _p(student), _p(target), _p(weight), n, fh, fw, q, eps, coef,
             _p(plane), _p(parts), _stream())
        res.append((parts.cpu().numpy(), plane.cpu().numpy() if with_plane else None))
    (parts, plane), (parts2, plane2), (parts3, _) = res
    assert np.isfinite(parts).all() and np.isfinite(plane).all()
    np.testing.assert_array_equal(parts.view(np.uint32), parts2.view(np.uint32))
    np.testing.assert_array_equal(plane.view(np.uint32), plane2.view(np.uint32))
    np.testing.assert_array_equal(parts.view(np.uint32), parts3.view(np.uint32))   # value only
    value = float(parts.astype(np.float64).sum())
    print("value %.6e ref %.6e" % (value, coef * S))
    if S == 0:                  # the degenerate record: weight 0 everywhere
        assert value == 0.0 and not plane.any()
        return
    assert abs(value - coef * S) <= REL_TOL * abs(coef * S)
    assert rel_l2(torch.from_numpy(plane), torch.from_numpy(coef * g)) < REL_TOL


def test_flow_distill_unaligned_views(lib):
    """Flows that are only 8-byte and a weight that is only 4-byte aligned take the one-cell
    path: the same values as the two-cell path."""
    from optical_flow_amd._lib import call
    c = SC.case((33, 65), "zoom")
    (fh, fw), n = c["grid"], SC.N
    total = n * fh * fw
    npart = lib.of_flow_distill_partials(n, fh, fw)
    outs = []
    for off in (0, 1):
        def shifted(a, width):
            buf = torch.zeros(total * width + 2 * width, device="cuda")
            v = buf[off * width:off * width + total * width]
            v.copy_(_dev(a).reshape(-1))
            return buf, v
        keep = [shifted(c["student"], 2), shifted(c["dtarget"], 2), shifted(c["dweight"], 1)]
        pbuf = _nan(total * 2 + 4)
        plane = pbuf[off * 2:off * 2 + total * 2]
        parts = _nan(npart)
        call("of_flow_distill_fwd", _p(keep[0][1]), _p(keep[1][1]), _p(keep[2][1]), n, fh, fw,
             0.4, 0.01, 1.0, _p(plane), _p(parts), _stream())
        outs.append((parts.cpu().numpy(), plane.cpu().numpy()))
        assert np.isnan(pbuf[:off * 2].cpu().numpy()).all()             # nothing outside the view
        assert np.isnan(pbuf[off * 2 + total * 2:].cpu().numpy()).all()
    np.testing.assert_array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32))
    np.testing.assert_array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32))


@pytest.mark.parametrize("q", [1.0, 0.4])
def test_selfsup_flow_loss_autograd(q):
    from optical_flow_amd import ops
    c = SC.case((33, 65), "rot")
    (fh, fw), n = c["grid"], SC.N
    S, g = R.distill(c["student"], c["dtarget"], c["dweight"], q, 0.01)
    flow = _dev(c["student"]).requires_grad_(True)
    loss = ops.selfsup_flow_loss(flow, _dev(c["dtarget"]), _dev(c["dweight"]), q, 0.01)
    (3.0 * loss).backward()
    cells = n * fh * fw
    assert abs(loss.item() - S / cells) <= REL_TOL * S / cells
    assert rel_l2(flow.grad, torch.from_numpy(3.0 * g / cells)) < REL_TOL


# ------------------------------------------------------------------------------ _Loss ----
def _loss_inputs():
    rng = np.random.default_rng(77)
    n, H, W = 2, 32, 48
    batch = _dev(rng.uniform(-0.5, 0.5, (n, H, W, 6)).astype(np.float32))
    flows = [_dev((rng.standard_normal((n, H >> (k + 1), W >> (k + 1), 2)) * 0.8)
                  .astype(np.float32)) for k in range(2)]
    target = _dev((rng.standard_normal((n, H // 2, W // 2, 2)) * 0.8).astype(np.float32))
    weight = _dev(rng.uniform(0, 1, (n, H // 2, W // 2)).astype(np.float32))
    return batch, flows, target, weight


def test_loss_is_additive():
    """photometric + census + self-supervision in one _Loss = the three stand-alone calls, the
    value and the flow gradients (the self-supervision term adds into level 0 alone)."""
    from optical_flow_amd import ops
    batch, flows, target, weight = _loss_inputs()

    def grads(fn):
        fl = [f.clone().requires_grad_(True) for f in flows]
        loss = fn(fl)
        loss.backward()
        return loss.item(), [f.grad for f in fl]

    both, gb = grads(lambda fl: ops.census_flow_loss(
        batch, fl, 0.7, 2, 1.0, convention="image", selfsup_weight=0.5, selfsup_q=0.4,
        selfsup_eps=0.01, selfsup=(target, weight)))
    p, gp = grads(lambda fl: ops.photometric_loss(batch, fl, "image"))
    c, gc = grads(lambda fl: ops.census_loss(batch, fl, 2, "image"))
    s, gs = grads(lambda fl: ops.selfsup_flow_loss(fl[0], target, weight, 0.4, 0.01) +
                  0.0 * fl[1].sum())
    want = p + 0.7 * c + 0.5 * s
    assert s > 0 and abs(both - want) <= REL_TOL * abs(want)
    for k in range(2):
        assert rel_l2(gb[k], gp[k] + 0.7 * gc[k] + 0.5 * gs[k]) < REL_TOL
    assert gs[0].abs().max() > 0
    # fewer target images than flow images: the first ones are scored, the rest get no gradient
    half, gh = grads(lambda fl: ops.census_flow_loss(
        batch, fl, 0.0, 2, 1.0, convention="image", selfsup_weight=0.5,
        selfsup=(target[:1], weight[:1])))
    s1, gs1 = grads(lambda fl: ops.selfsup_flow_loss(fl[0][:1], target[:1], weight[:1]) +
                    0.0 * fl[1].sum())
    assert abs(half - (p + 0.5 * s1)) <= REL_TOL * abs(p + 0.5 * s1)
    assert rel_l2(gh[0], gp[0] + 0.5 * gs1[0]) < REL_TOL


def test_ninth_group_raises():
    """of_sum_partials takes 8 groups: five photometric levels + census + SSIM + smoothness +
    self-supervision would be nine."""
    from optical_flow_amd import ops
    n, H = 1, 96                                    # levels 48, 24, 12, 6, 3
    batch = torch.zeros(n, H, H, 6, device="cuda")
    flows = [torch.zeros(n, H >> (k + 1), H >> (k + 1), 2, device="cuda") for k in range(5)]
    sup = (torch.zeros(n, 48, 48, 2, device="cuda"), torch.ones(n, 48, 48, device="cuda"))
    with pytest.raises(ValueError, match="8 groups"):
        ops.census_flow_loss(batch, flows, 1.0, 1, 1.0, smoothness_weight=0.1, convention="image",
                             ssim_weight=0.5, selfsup_weight=0.5, selfsup=sup)
    # eight fit
    loss = ops.census_flow_loss(batch, flows, 1.0, 1, 1.0, convention="image", ssim_weight=0.5,
                                selfsup_weight=0.5, selfsup=sup)
    assert torch.isfinite(loss).item()


# ---------------------------------------------------------------------------- Trainer ----
TH, TW, TB = 64, 128, 2


def _trainer(occlusion="none", selfsup=True, seed=0):
    from optical_flow_amd.data_reader import AugmentOpts
    from optical_flow_amd.loss import LossLayer
    from optical_flow_amd.model import FlowNet
    from optical_flow_amd.train import KerasAdam, Trainer
    net = FlowNet(TH, TW, seed=seed, warp_convention="image")
    layer = LossLayer(warp_convention="image", occlusion=occlusion,
                      selfsup_weight=0.3 if selfsup else 0.0)
    opts = AugmentOpts(zoom=(1.0, 1.3), hflip_prob=0.5, brightness=0.1) if selfsup else None
    return Trainer(net, KerasAdam(net.store), layer, data_parallel=False, selfsup=opts,
                   selfsup_seed=5)


def _batch(seed=23):
    from optical_flow_amd.data import synthetic_batch
    return torch.from_numpy(synthetic_batch(TB, TH, TW, seed=seed)).cuda()


def _identity_records():
    return np.array([R.identity(TH, TW)] * TB)


@pytest.mark.parametrize("occlusion", ["none", "border", "fb"])
def test_trainer_selfsup_step(occlusion):
    """One self-supervised step: the teacher pass touches nothing, the step trains, and under
    identity records last_selfsup is what the restatement makes of the teacher's flow."""
    tr = _trainer(occlusion)
    store = tr.flow_net.store
    batch = _batch()
    tr.flow_net(batch)                                   # packs the weights, builds the guard
    store.zero_grad()
    before = [store.arena.clone(), store.grad_arena.clone(), store.buffers.clone()]
    version = store.version
    teacher, mask = tr.teacher_pass(batch)
    torch.cuda.synchronize()
    assert store.version == version
    for a, b in zip(before, (store.arena, store.grad_arena, store.buffers)):
        assert torch.equal(a, b)
    assert teacher.shape == (TB, TH // 2, TW // 2, 2) and not teacher.requires_grad
    assert (mask is None) == (occlusion == "none")
    if mask is not None:
        assert mask.shape == (TB, TH // 2, TW // 2)

    loss, flows = tr.train_step(batch, 0, selfsup_records=_identity_records())
    assert torch.isfinite(loss).item()
    assert not torch.equal(before[0], store.arena)       # the weights moved
    assert [tuple(f.shape) for f in flows] == [(TB, TH >> (k + 1), TW >> (k + 1), 2)
                                               for k in range(4)]
    last = tr.last_selfsup
    # 64 x 128: the identity record is exact, the augmented batch is the batch
    assert torch.equal(last["batch"], batch)
    tref, wref = R.transform_flow(teacher.cpu().numpy(), _identity_records(), (TH, TW),
                                  None if mask is None else mask.cpu().numpy())
    assert rel_l2(last["target"], torch.from_numpy(tref)) < REL_TOL
    ik, vk = R.near_kink(teacher.cpu().numpy(), _identity_records(), (TH, TW))
    ok = ~vk                     # (the identity is exact at this size: no inside kink decides)
    assert np.abs(last["weight"].cpu().numpy() - wref)[ok].max() <= REL_TOL
    assert last["records"].dtype == torch.uint8 and last["records"].numel() == TB * 64

    # a seeded step with the trainer's own records
    loss2, _ = tr.train_step(batch, 1)
    assert torch.isfinite(loss2).item()
    assert not torch.equal(tr.last_selfsup["batch"], batch)
    assert 0 < tr.last_selfsup["weight"].mean().item() <= 1


def test_trainer_selfsup_disabled_is_the_plain_step():
    a, b = _trainer(selfsup=True), _trainer(selfsup=False)
    assert torch.equal(a.flow_net.store.arena, b.flow_net.store.arena)
    a.selfsup_enabled = False
    batch = _batch()
    for step in range(2):
        la, fa = a.train_step(batch, step)
        lb, fb = b.train_step(batch, step)
        assert torch.equal(la, lb)
        for x, y in zip(fa, fb):
            assert torch.equal(x, y)
    assert torch.equal(a.flow_net.store.arena, b.flow_net.store.arena)
    assert a.last_selfsup is None
    with pytest.raises(ValueError, match="self-supervision is off"):
        a.train_step(batch, 2, selfsup_records=_identity_records())


def test_trainer_refusals():
    from optical_flow_amd.data_reader import AugmentOpts
    from optical_flow_amd.loss import LossLayer
    from optical_flow_amd.model import FlowNet
    from optical_flow_amd.train import Trainer
    tr = _trainer()
    with pytest.raises(RuntimeError, match="self-supervised"):
        tr.graphed(_batch())
    net = tr.flow_net
    with pytest.raises(ValueError, match="trainer needs the augmentation"):
        Trainer(net, None, LossLayer(warp_convention="image", selfsup_weight=0.3),
                data_parallel=False)
    with pytest.raises(ValueError, match="selfsup_weight is 0"):
        Trainer(net, None, LossLayer(warp_convention="image"), data_parallel=False,
                selfsup=AugmentOpts(hflip_prob=0.5))
    bn = FlowNet(TH, TW, seed=0, warp_convention="image", bn_mode="training")
    with pytest.raises(ValueError, match="moving statistics"):
        Trainer(bn, None, LossLayer(warp_convention="image", selfsup_weight=0.3),
                data_parallel=False, selfsup=AugmentOpts(hflip_prob=0.5))
