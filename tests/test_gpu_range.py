"""Range-map occlusion on the device (DESIGN.md "Range-map occlusion"; include/oflow.h
of_occ_range_multi): the three kernels through the C ABI against the float64 restatement in
tests/range_ref.py, exact known answers, reproducibility, partner wiring, non-finite and far
flows, the OF_EINVAL cases, ops.range_map / ops.occlusion_masks(..., "range"),
LossLayer(occlusion="range") and a whole train step, eager and captured.

Tolerance of R and of the mask: absolute 1e-5.  Per landed tap the fp32 weight (fx exact, one
rounding in 1 - fx, one in the product, per axis) is within 2e-7 of the float64 weight and the
quantisation to 2^-24 adds 2^-25 = 3e-8; at most 32 taps land on a pixel
(tests/test_range_host.py asserts it for these inputs), so the sum is within 32 * 2.3e-7 =
7.4e-6.  The mask is compared on every pixel that is not within 1e-4 of a border decision (the
host test shows there is none)."""
import ctypes as C
import functools

import pytest
import torch

import occlusion_ref as O
import range_ref as RR
from helpers import REL_TOL, dev, f64, rel_l2
from test_gpu_occlusion import LAYERS, _arr, _hw, _masks, _ptrs, _rel
from test_gpu_smooth_loss import ref_smooth

pytestmark = pytest.mark.gpu

NAN = float("nan")
ABS_TOL = 1e-5
SENTINEL = 0x5A5A5A5A5A5A5A5A


def _status(flows, n, stride, levels, ranges="new", masks="new", ws="new", ws_bytes=None,
            nlevels=None, null_flows=False):
    """of_occ_range_multi's status with NaN-prefilled outputs and a sentinel-filled workspace:
    (status, ranges, masks, workspace).  ``ranges`` / ``masks`` None: a NULL array."""
    from optical_flow_amd import _lib, ops
    shape = [(max(n, 1), h, w) for h, w in levels]
    if ranges == "new":
        ranges = [torch.full(s, NAN, device="cuda") for s in shape]
    if masks == "new":
        masks = [torch.full(s, NAN, device="cuda") for s in shape]
    if isinstance(ws, str):
        ws = torch.full((sum(a * b * c for a, b, c in shape) + 1,), SENTINEL, dtype=torch.int64,
                        device="cuda")
    hs, wsz = _hw(levels)
    L = len(levels) if nlevels is None else nlevels
    if ws_bytes is None:
        ws_bytes = 8 * sum(max(n, 0) * h * w for h, w in levels)
    wptr = ws if isinstance(ws, int) or ws is None else ws.data_ptr()
    st = _lib.lib().of_occ_range_multi(
        None if null_flows else _ptrs(flows), n, stride, hs, wsz, L, wptr, ws_bytes,
        _ptrs(ranges) if ranges is not None else None,
        _ptrs(masks) if masks is not None else None, ops._stream())
    torch.cuda.synchronize()
    return st, ranges, masks, ws


def _range(flows):
    """(ranges, masks) of device flows through the C ABI."""
    from optical_flow_amd import _lib
    n = flows[0].shape[0]
    levels = [(f.shape[1], f.shape[2]) for f in flows]
    st, ranges, masks, _ = _status(flows, n, n // 2, levels)
    assert st == 0, _lib.lib().of_last_error()
    return ranges, masks


@functools.lru_cache(maxsize=None)
def _abi():
    """The ABI inputs, their float64 references and the device results (computed once)."""
    flows = RR.abi_flows()
    want = [(RR.range_map(f64(f)), RR.mask(f64(f)), RR.near(f64(f), "border")) for f in flows]
    fd = [dev(f) for f in flows]
    return flows, fd, want, _range(fd)


# --------------------------------------------------------------------------- 1. the ABI ----
def test_range_kernel_abi():
    """Four levels (1 x 1, under a block, ragged, several blocks) in one launch, n = 4: every
    element written (NaN prefill), R and the mask within 1e-5 of the reference."""
    flows, _, want, (ranges, masks) = _abi()
    for f, (wr, wm, nr), r, m in zip(flows, want, ranges, masks):
        r, m = r.cpu().double(), m.cpu().double()
        assert torch.isfinite(r).all() and torch.isfinite(m).all()
        er, em = (r - wr).abs().max().item(), ((m - wm).abs() * ~nr).max().item()
        print(tuple(f.shape), "max |R - ref| %.2e  max |mask - ref| %.2e  near %d  mean mask %.3f"
              % (er, em, int(nr.sum()), m.mean().item()))
        assert (r >= 0).all() and (m >= 0).all() and (m <= 1).all()
        assert er <= ABS_TOL and em <= ABS_TOL


@pytest.mark.parametrize("name", ["zero", "shift", "contract", "expand"])
def test_known_answers_are_exact(name):
    """Every tap weight is 0, 0.25, 0.5 or 1, exact in 2^-24 units: the device result equals
    the float64 reference bit for bit (the host test asserts the reference's values)."""
    h, w, B = 13, 21, 2
    f = RR.known_flows(h, w, B)[name]
    (r,), (m,) = _range([dev(f)])
    r, m = r.cpu().double(), m.cpu().double()
    assert torch.equal(r, RR.range_map(f64(f)))
    assert torch.equal(m, RR.mask(f64(f)))
    if name == "zero":
        assert (r == 1.0).all() and (m == 1.0).all()
    elif name == "shift":
        assert torch.equal(m, O.border(f64(f))[0])
        assert (m[:B, :, w - 2:] == 0).all() and (m[B:, :, :2] == 0).all()
        assert m.sum() == 4 * h * (w - 2)
    elif name == "contract":
        assert (r[:B, 1:(h - 2) // 2 + 1, 1:(w - 2) // 2 + 1] == 4.0).all()
        assert (r[:B, 0, 0] == 2.25).all() and (r[:B, h - 1, w - 1] == 0.0).all()
    else:
        want = torch.zeros(h, w, dtype=torch.float64)
        want[0::2, 0::2] = 1.0
        assert torch.equal(r[0], want) and torch.equal(r[1], want)


def test_two_calls_give_equal_bits():
    """Integer accumulation: a second call on the same input gives the same bits."""
    _, fd, _, (ranges, masks) = _abi()
    ranges2, masks2 = _range(fd)
    for a, b in zip(ranges + masks, ranges2 + masks2):
        assert torch.equal(a, b)


def test_partner_wiring():
    """Exchanging the two pairs' backward flows changes the forward masks (image b receives
    from b + B, not from some other image), as the reference says it does."""
    _, fd, _, (_, masks) = _abi()
    B = RR.ABI_N // 2
    swapped = [torch.cat([f[:B], f[B:].flip(0)], 0).contiguous() for f in fd]
    _, other = _range(swapped)
    for l in (2, 3):
        assert not torch.equal(other[l][:B], masks[l][:B])
        want = RR.mask(f64(swapped[l]))
        assert (other[l].cpu().double() - want).abs().max().item() <= ABS_TOL


def test_non_finite_and_far_flows():
    """NaN, +-inf and +-1e9 at a few source pixels: every output finite and equal to the
    reference with those sources dropped (no tap of theirs lands anywhere)."""
    bad, clean, keep = RR.edge_flows()
    (r,), (m,) = _range([dev(bad)])
    r, m = r.cpu().double(), m.cpu().double()
    assert torch.isfinite(r).all() and torch.isfinite(m).all()
    wr = RR.range_map(f64(clean), keep)
    wm = O.border(f64(bad))[0] * wr.clamp(max=1.0)
    nr = RR.near(f64(bad), "border")
    er, em = (r - wr).abs().max().item(), ((m - wm).abs() * ~nr).max().item()
    print("max |R - ref| %.2e  max |mask - ref| %.2e  near %d" % (er, em, int(nr.sum())))
    assert er <= ABS_TOL and em <= ABS_TOL
    assert (m[~keep] == 0).all()                        # their own sample is not in the frame


def test_einval_launches_nothing():
    from optical_flow_amd import _lib
    levels = [(5, 3), (13, 21)]
    flows = [torch.zeros(4, h, w, 2, device="cuda") for h, w in levels]
    ok = dict(flows=flows, n=4, stride=2, levels=levels)
    off4 = [torch.zeros(4 * h * w * 2 + 1, device="cuda")[1:] for h, w in levels]   # 4 mod 8
    assert all(t.data_ptr() % 8 == 4 for t in off4)
    wsbuf = torch.full((4 * (15 + 273) + 1,), SENTINEL, dtype=torch.int64, device="cuda")
    bad = [dict(nlevels=0), dict(nlevels=9), dict(n=0, stride=0), dict(n=1, stride=1),
           dict(n=1, stride=0), dict(stride=1), dict(stride=4), dict(n=3, stride=1),
           dict(n=-2, stride=-1), dict(levels=[(5, 3), (0, 21)]), dict(levels=[(5, 0), (13, 21)]),
           dict(levels=[(5, 3), (1 << 20, 1 << 20)]), dict(null_flows=True),
           dict(flows=[flows[0], None]), dict(flows=[flows[0], off4[1]]), dict(ws=None),
           dict(ws=wsbuf.data_ptr() + 4), dict(ws_bytes=8 * 4 * (15 + 273) - 8), dict(ws_bytes=0),
           dict(ranges=None, masks=None)]
    for kw in bad:
        outs = [[torch.full((4, 5, 3), NAN, device="cuda"),
                 torch.full((4, 13, 21), NAN, device="cuda")] for _ in range(2)]
        args = {**ok, "ranges": outs[0], "masks": outs[1], "ws": wsbuf, **kw}
        st, _, _, _ = _status(**args)
        assert st == _lib.OF_EINVAL, kw
        assert _lib.lib().of_last_error().startswith(b"of_occ_range_multi"), kw
        assert all(torch.isnan(o).all() for o in outs[0] + outs[1]), kw
        assert (wsbuf == SENTINEL).all(), kw
    # the workspace query: 8 bytes per pixel, 0 for what the entry rejects
    q = _lib.lib().of_occ_range_ws_bytes
    hs, ws = _hw(levels)
    assert q(4, hs, ws, 2) == 8 * 4 * (15 + 273)
    assert q(1, hs, ws, 2) == 0 and q(4, hs, ws, 0) == 0 and q(4, hs, ws, 9) == 0
    assert q(4, None, ws, 2) == 0 and q(4, *_hw([(5, 3), (0, 21)]), 2) == 0
    assert q(4, *_hw([(5, 3), (1 << 20, 1 << 20)]), 2) == 0
    # legal: both outputs, ranges alone, masks alone, a NULL entry; the workspace's last word
    # (past of_occ_range_ws_bytes) stays untouched
    st, r, m, w = _status(**ok)
    assert st == 0 and all((o == 1.0).all() for o in r + m) and w[-1] == SENTINEL
    st, r, _, _ = _status(**ok, masks=None)
    assert st == 0 and all((o == 1.0).all() for o in r)
    st, _, m, _ = _status(**ok, ranges=None)
    assert st == 0 and all((o == 1.0).all() for o in m)
    st, r, m, _ = _status(**ok, ranges=[None, torch.full((4, 13, 21), NAN, device="cuda")])
    assert st == 0 and (r[1] == 1.0).all() and all((o == 1.0).all() for o in m)


# ------------------------------------------------------------------------------ 2. ops ----
def test_ops_range_map_and_masks():
    """ops.range_map and ops.occlusion_masks(flows, "range") are the ABI's results, plain
    tensors without autograd; the alphas are ignored."""
    from optical_flow_amd import ops
    flows, fd, _, (ranges, masks) = _abi()
    req = [f.clone().requires_grad_(True) for f in fd]
    got_r = ops.range_map(req)
    got_m = ops.occlusion_masks(req, "range")
    got_a = ops.occlusion_masks(req, "range", 0.3, 7.0, "image")
    for f, r, m, a, wr, wm in zip(flows, got_r, got_m, got_a, ranges, masks):
        for t in (r, m):
            assert t.shape == f.shape[:3] and t.dtype == torch.float32 and not t.requires_grad
        assert torch.equal(r, wr) and torch.equal(m, wm) and torch.equal(a, wm)


@pytest.mark.parametrize("mode", ["border", "fb"])
def test_other_modes_are_untouched(mode):
    """ops.occlusion_masks with "border" and "fb" still returns, bit for bit, what
    of_occ_mask_multi gives when called directly with alpha2 / 4^(s+1) per level."""
    from optical_flow_amd import ops
    fd = [dev(f) for f in O.abi_flows(mode)]
    a1, a2 = 0.02, 0.25
    got = ops.occlusion_masks(fd, mode, a1, a2)
    want = _masks(fd, mode, [a2 / 4.0 ** (s + 1) for s in range(len(fd))], a1)
    for g, w in zip(got, want):
        assert ((g == 0.0) | (g == 1.0)).all() and torch.equal(g, w)


# ------------------------------------------------------------------------ 3. LossLayer ----
@functools.lru_cache(maxsize=None)
def _layer_ref():
    """The LossLayer case and, in float64, the reference range masks and the three terms with
    their d(flow): masked photometric, masked census (r = 3), smoothness (alpha 10)."""
    batch, flows = RR.layer_case()
    b = f64(batch)
    masks = RR.masks([f64(f) for f in flows])
    terms = []
    for fn in (lambda fo: RR.photometric(b, fo, masks), lambda fo: RR.census(b, fo, 3, masks),
               lambda fo: ref_smooth(b, fo, 10.0)):
        fo = [f64(f).requires_grad_(True) for f in flows]
        v = fn(fo)
        terms.append((v.item(), torch.autograd.grad(v, fo)))
    return batch, flows, masks, terms


@pytest.mark.parametrize("which", list(LAYERS))
def test_loss_layer_with_range(which):
    """LossLayer(occlusion="range"): the loss and every d(flow) against the reference
    composition with the (detached) reference masks."""
    from optical_flow_amd.loss import LossLayer
    batch, flows, _, terms = _layer_ref()
    kw, mix = LAYERS[which]
    want = sum(c * t[0] for c, t in zip(mix, terms))
    grads = [sum(c * t[1][s] for c, t in zip(mix, terms)) for s in range(len(flows))]
    fd = [dev(f).requires_grad_(True) for f in flows]
    loss = LossLayer(warp_convention="image", occlusion="range", **kw)(dev(batch), fd)
    loss.backward()
    errs = [rel_l2(f.grad, g) for f, g in zip(fd, grads)]
    print(which, loss.item(), want, "d(flow)", errs)
    assert loss.shape == () and _rel(loss.item(), want) < REL_TOL
    assert max(errs) < REL_TOL, errs


# ------------------------------------------------------------------------------ 4. step ----
NET_SEED, BATCH_SEED = 0, 1236


def _range_trainer():
    from optical_flow_amd.loss import LossLayer
    from optical_flow_amd.model import build_flow_net
    from optical_flow_amd.train import Trainer
    net = build_flow_net(64, 64, seed=NET_SEED, levels=4, warp_convention="image")
    layer = LossLayer(0.2, 10, census_weight=1.0, photometric_weight=0.0,
                      warp_convention="image", occlusion="range")
    return Trainer(net, loss_layer=layer)


def _batch():
    from optical_flow_amd.data import synthetic_batch
    return dev(torch.from_numpy(synthetic_batch(2, 64, 64, seed=BATCH_SEED)))


def test_range_train_step():
    """Trainer.train_step with occlusion="range" at 64 x 64, B = 2: the net runs on the doubled
    batch, the loss is finite, the returned flows have batch B; a second trainer from the same
    seed: loss, flows and parameters bitwise equal."""
    batch = _batch()
    res = []
    for _ in range(2):
        trainer = _range_trainer()
        loss, flows = trainer.train_step(batch)
        torch.cuda.synchronize()
        assert torch.isfinite(loss).all()
        assert [tuple(f.shape) for f in flows] == [(2, 64 >> (s + 1), 64 >> (s + 1), 2)
                                                   for s in range(4)]
        assert all(torch.isfinite(f).all() for f in flows)
        store = trainer.flow_net.store
        assert torch.isfinite(store.grad_arena).all() and store.grad_arena.abs().max() > 0
        res.append((loss.clone(), [f.clone() for f in flows], store.arena.clone()))
    assert torch.equal(res[0][0], res[1][0])
    assert all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1]))
    assert torch.equal(res[0][2], res[1][2])


def test_selfsup_step_carries_the_soft_mask():
    """Self-supervision with occlusion="range": the teacher pass runs on the doubled batch and
    returns the level-0 range mask of the first B images, a soft weight; the step's target and
    weight are what the restatement makes of them (test_gpu_selfsup's own check of a step, whose
    transform carries any mask bilinearly)."""
    import test_gpu_selfsup as S
    from optical_flow_amd import ops
    tr, batch = S._trainer("range"), S._batch()
    teacher, mask = tr.teacher_pass(batch)
    doubled = torch.cat([batch, torch.cat([batch[..., 3:], batch[..., :3]], -1)], 0)
    with torch.no_grad():
        want = ops.occlusion_masks(tr.flow_net(doubled), "range")[0][:S.TB]
    assert teacher.shape == (S.TB, S.TH // 2, S.TW // 2, 2) and torch.equal(mask, want)
    assert (mask >= 0).all() and (mask <= 1).all() and ((mask > 0) & (mask < 1)).any()
    S.test_trainer_selfsup_step("range")


def test_range_step_captures():
    """trainer.graphed captures the range step (the doubled batch, the workspace and the three
    range kernels inside the capture); a replay's loss equals the eager step's on the same
    weights and batch, and the replay returns forward flows of batch B."""
    from test_gpu_graph import _sync_state
    batch = _batch()
    gt, eager = _range_trainer(), _range_trainer()
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
