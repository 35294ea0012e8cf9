"""The loss's launch sequences and its FlowGrad protocol (DESIGN.md "The loss Function"): which
C entry points each public loss entry calls, in which order and with which ``accumulate``, for
every combination of terms; that the entries of the training loss write a flow head's gradient
buffer and the two stand-alone terms never do; the seven-level census + smoothness loss; that
all six terms in one Function add up to the six stand-alone calls; and what each term saves
for its backward.

Shapes: n = 2, a 32 x 32 batch and four flows of 16 x 16 down to 2 x 2, the smallest at which
every branch exists (a level smaller than the census window, one with a single pair per
direction)."""
import functools

import pytest
import torch

from helpers import REL_TOL, dev, rel_l2, rng_tensor

pytestmark = pytest.mark.gpu

N, S, LEVELS = 2, 32, 4
BWD_WITH_ACC = ("of_census_bwd_multi", "of_flow_smooth_bwd_multi", "of_ssim_bwd_multi",
                "of_flow_smooth2_bwd_multi")


@functools.lru_cache(maxsize=None)
def _inputs(n=N, size=S, levels=LEVELS):
    from optical_flow_amd.data import synthetic_batch
    batch = dev(torch.from_numpy(synthetic_batch(n, size, size, seed=5)))
    flows = [rng_tensor((n, size >> (s + 1), size >> (s + 1), 2), 50 + s, scale=2.0)
             for s in range(levels)]
    return batch, flows


@functools.lru_cache(maxsize=None)
def _labels(n=N, size=S, levels=LEVELS):
    """Two small KITTI-format uint16 maps around the finest flow (test_gpu_supervised.py's
    recipe) and a self-supervision (target, weight) pair on the finest grid."""
    import numpy as np

    import kitti_flow_np as K
    import supervised_ref as R
    f0 = _inputs(n, size, levels)[1][0].numpy()
    rng = np.random.default_rng(31)
    maps = [R.make_gt(K.upsample_np(f0[i], gh, gw), rng)
            for i, (gh, gw) in enumerate([(37, 61), (33, 67)][:n])]
    target = dev(rng_tensor(f0.shape, 60, scale=2.0))
    weight = dev(rng_tensor(f0.shape[:3], 61, lo=0.0, hi=1.0))
    return maps, (target, weight)


def _ones(flows):
    return [torch.ones(f.shape[:3], device="cuda") for f in flows]


def _three(ops, b, f, **kw):
    return ops.census_flow_loss(b, f, 0.5, 3, 0.5, 0.2, 10, **kw)


PYR, SUM = "of_pyramid6", "of_sum_partials"
PF, PB = "of_photo_l1_fwd_multi", "of_photo_l1_bwd_multi"
CF, SF = "of_census_fwd_multi", "of_flow_smooth_fwd_multi"
CB0, CB1 = "of_census_bwd_multi(acc 0)", "of_census_bwd_multi(acc 1)"
SB0, SB1 = "of_flow_smooth_bwd_multi(acc 0)", "of_flow_smooth_bwd_multi(acc 1)"

SSF, SUPF, DF = "of_ssim_fwd_multi", "of_supervised_fwd_multi", "of_flow_distill_fwd"
SSB0, SSB1 = "of_ssim_bwd_multi(acc 0)", "of_ssim_bwd_multi(acc 1)"
S2F = "of_flow_smooth2_fwd_multi"
S2B0, S2B1 = "of_flow_smooth2_bwd_multi(acc 0)", "of_flow_smooth2_bwd_multi(acc 1)"
# the supervised and the self-supervision planes go through of_census_bwd_multi; the
# self-supervision term's launch holds level 0 alone
CB0_L0, CB1_L0 = "of_census_bwd_multi(acc 0, 1 level)", "of_census_bwd_multi(acc 1, 1 level)"

# id: (call, forward names, backward names)
ROWS = {
    "photometric": (lambda ops, b, f: ops.photometric_loss(b, f),
                    [PYR, PF, SUM], [PB]),
    "photometric_image": (lambda ops, b, f: ops.photometric_loss(b, f, convention="image"),
                          [PYR, PF + "_cv", SUM], [PB + "_cv"]),
    "flow_loss": (lambda ops, b, f: ops.flow_loss(b, f, 0.2, 10),
                  [PYR, PF, SF, SUM], [PB, SB1]),
    # a zero weight launches nothing: what photometric_loss launches
    "flow_loss_weight0": (lambda ops, b, f: ops.flow_loss(b, f, 0.0),
                          [PYR, PF, SUM], [PB]),
    "smoothness_alpha0": (lambda ops, b, f: ops.flow_smoothness(b, f, edge_alpha=0),
                          [SF, SUM], [SB0]),
    "smoothness_alpha10": (lambda ops, b, f: ops.flow_smoothness(b, f, edge_alpha=10),
                           [PYR, SF, SUM], [SB0]),
    "census": (lambda ops, b, f: ops.census_loss(b, f),
               [PYR, CF, SUM], [CB0]),
    "three_terms": (_three, [PYR, PF, CF, SF, SUM], [PB, CB1, SB1]),
    "census_smoothness": (lambda ops, b, f: ops.census_flow_loss(b, f, 0.5, 3, 0.0, 0.2, 10),
                          [PYR, CF, SF, SUM], [CB0, SB1]),
    "three_terms_image_weights": (
        lambda ops, b, f: _three(ops, b, f, convention="image", weights=_ones(f)),
        [PYR, PF + "_w", CF + "_w", SF, SUM], [PB + "_w", CB1, SB1]),
    "ssim": (lambda ops, b, f: ops.ssim_loss(b, f),
             [PYR, SSF, SUM], [SSB0]),
    "four_terms_ssim": (lambda ops, b, f: _three(ops, b, f, ssim_weight=0.3),
                        [PYR, PF, CF, SSF, SF, SUM], [PB, CB1, SSB1, SB1]),
    "four_terms_ssim_image_weights": (
        lambda ops, b, f: _three(ops, b, f, convention="image", weights=_ones(f),
                                 ssim_weight=0.3),
        [PYR, PF + "_w", CF + "_w", SSF, SF, SUM], [PB + "_w", CB1, SSB1, SB1]),
    "supervised": (lambda ops, b, f: ops.supervised_flow_loss(f, _labels()[0]),
                   [SUPF, SUM], [CB0]),
    "three_terms_supervised": (
        lambda ops, b, f: _three(ops, b, f, convention="image", supervised_weight=0.7,
                                 gt=_labels()[0]),
        [PYR, PF + "_cv", CF + "_cv", SUPF, SF, SUM], [PB + "_cv", CB1, CB1, SB1]),
    "selfsup": (lambda ops, b, f: ops.selfsup_flow_loss(f[0], *_labels()[1]),
                [DF, SUM], [CB0_L0]),
    "three_terms_selfsup": (
        lambda ops, b, f: _three(ops, b, f, convention="image", selfsup_weight=0.5,
                                 selfsup=_labels()[1]),
        [PYR, PF + "_cv", CF + "_cv", DF, SF, SUM], [PB + "_cv", CB1, CB1_L0, SB1]),
    "smoothness2_alpha10": (lambda ops, b, f: ops.flow_smoothness(b, f, edge_alpha=10, order=2),
                            [PYR, S2F, SUM], [S2B0]),
    "flow_loss_order2": (lambda ops, b, f: ops.flow_loss(b, f, 0.2, 10, smoothness_order=2),
                         [PYR, PF, S2F, SUM], [PB, S2B1]),
}


def _spy(monkeypatch, ops):
    called = []
    real = ops.call

    def call(name, *a):
        # accumulate is the argument before the stream; of_census_bwd_multi's fifth argument
        # is its level count
        if name == "of_census_bwd_multi" and a[4] != LEVELS:
            called.append("%s(acc %d, %d level)" % (name, a[-2], a[4]))
        else:
            called.append("%s(acc %d)" % (name, a[-2]) if name in BWD_WITH_ACC else name)
        return real(name, *a)
    monkeypatch.setattr(ops, "call", call)
    return called


@pytest.mark.parametrize("grad", [True, False], ids=["grad", "nograd"])
@pytest.mark.parametrize("row", list(ROWS))
def test_launch_sequence(monkeypatch, row, grad):
    """One forward and one backward: the entry names in order.  With no flow requiring grad
    there is no backward, and nothing follows of_sum_partials."""
    from optical_flow_amd import ops
    fn, fwd, bwd = ROWS[row]
    batch, flows = _inputs()
    fd = [dev(f).requires_grad_(grad) for f in flows]
    called = _spy(monkeypatch, ops)
    loss = fn(ops, batch, fd)
    assert called == fwd
    assert loss.requires_grad == grad
    if grad:
        loss.backward()
        assert called == fwd + bwd
    torch.cuda.synchronize()
    assert called == fwd + (bwd if grad else [])


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


@pytest.mark.parametrize("row", ["photometric", "flow_loss", "three_terms"])
def test_training_entries_fill_the_flowgrads(row):
    """A flow that carries a FlowGrad gets its gradient in that buffer: filled, bitwise the
    plain gradient, channels 2-3 exactly 0."""
    from optical_flow_amd import ops
    fn = ROWS[row][0]
    batch, flows = _inputs()
    plain, _ = _grads(fn, ops, batch, flows, False)
    routed, fgs = _grads(fn, ops, batch, flows, True)
    try:
        for g, p, fg in zip(routed, plain, fgs):
            assert fg.filled
            assert torch.equal(g, p)
            assert torch.equal(fg.buffer()[..., :2], p)
            assert (fg.buffer()[..., 2:] == 0).all()
    finally:
        for fg in fgs:
            fg.release()


@pytest.mark.parametrize("row", ["census", "smoothness_alpha0", "smoothness_alpha10"])
def test_standalone_terms_leave_the_flowgrads_alone(row):
    """census_loss and flow_smoothness return plain gradients even for flows that carry a
    FlowGrad: nothing is marked filled, the gradients are bitwise the plain ones."""
    from optical_flow_amd import ops
    fn = ROWS[row][0]
    batch, flows = _inputs()
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


def test_seven_levels_census_and_smoothness():
    """census + smoothness without the photometric term needs two sum groups, so it takes seven
    levels (128 x 128, flows of 64 x 64 down to 1 x 1): the loss and every d(flow) against
    0.7 * census_loss + 0.2 * flow_smoothness.  Tolerance 1e-5: the two sides differ by a few
    fp32 roundings of one extra add and multiply.  A level whose reference gradient is exactly
    zero (1 x 1: no pairs, a window of one) must be exactly zero."""
    from optical_flow_amd import ops
    batch, flows = _inputs(1, 128, 7)
    assert flows[-1].shape == (1, 1, 1, 2)
    fr = [dev(f).requires_grad_(True) for f in flows]
    ref = (0.7 * ops.census_loss(batch, fr, radius=1) +
           0.2 * ops.flow_smoothness(batch, fr, edge_alpha=10))
    ref.backward()
    fd = [dev(f).requires_grad_(True) for f in flows]
    loss = ops.census_flow_loss(batch, fd, census_weight=0.7, census_radius=1,
                                photometric_weight=0, smoothness_weight=0.2, edge_alpha=10)
    loss.backward()
    torch.cuda.synchronize()
    errs = [rel_l2(a.grad, b.grad) for a, b in zip(fd, fr)]
    print("loss", loss.item(), ref.item(), "d(flow) rel_l2", errs)
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())
    for a, b, e in zip(fd, fr, errs):
        if not b.grad.any():
            assert torch.equal(a.grad, b.grad)
        else:
            assert e < 1e-5, errs


# ------------------------------------------------------------------- all six terms ----
@functools.lru_cache(maxsize=None)
def _six_inputs():
    """n = 2, a 32 x 48 batch, levels of 16 x 24 and 8 x 12; ground truth and a self-supervision
    pair for the first image only."""
    import numpy as np

    import kitti_flow_np as K
    import supervised_ref as R
    from optical_flow_amd.data import synthetic_batch
    batch = dev(torch.from_numpy(synthetic_batch(2, 32, 48, seed=6)))
    flows = [rng_tensor((2, 32 >> (s + 1), 48 >> (s + 1), 2), 70 + s, scale=0.8) for s in range(2)]
    maps = [R.make_gt(K.upsample_np(flows[0][0].numpy(), 37, 61), np.random.default_rng(32))]
    target = dev(rng_tensor((1, 16, 24, 2), 72, scale=0.8))
    weight = dev(rng_tensor((1, 16, 24), 73, lo=0.0, hi=1.0))
    return batch, flows, maps, (target, weight)


SIX_W = dict(photo=0.9, census=0.7, ssim=0.6, sup=0.5, selfsup=0.4, smooth=0.3)


def _six(ops, batch, fl, maps, pair):
    return ops.census_flow_loss(
        batch, fl, SIX_W["census"], 2, SIX_W["photo"], SIX_W["smooth"], 10.0,
        convention="image", ssim_weight=SIX_W["ssim"], supervised_weight=SIX_W["sup"],
        supervised_q=0.4, gt=maps, selfsup_weight=SIX_W["selfsup"], selfsup_q=0.4,
        selfsup=pair, smoothness_order=2)


def test_six_terms_are_additive():
    """All six terms in one _Loss (two photometric groups + five = seven sum groups) against the
    weighted sum of the six stand-alone calls: the value and each level's gradient, within
    test_gpu_selfsup.py's test_loss_is_additive tolerance; and with FlowGrads attached the
    gradients are bitwise the plain ones."""
    from optical_flow_amd import ops
    batch, flows, maps, pair = _six_inputs()

    def grads(fn, attach=False):
        fl = [dev(f).requires_grad_(True) for f in flows]
        fgs = []
        if attach:
            for f in fl:
                f._of_flowgrad = ops.FlowGrad(f.shape, f.device)
                fgs.append(f._of_flowgrad)
        loss = fn(fl)
        loss.backward()
        torch.cuda.synchronize()
        return loss.item(), [f.grad for f in fl], fgs

    both, gb, _ = grads(lambda fl: _six(ops, batch, fl, maps, pair))
    alone = {
        "photo": lambda fl: ops.photometric_loss(batch, fl, "image"),
        "census": lambda fl: ops.census_loss(batch, fl, 2, "image"),
        "ssim": lambda fl: ops.ssim_loss(batch, fl, "image"),
        "sup": lambda fl: ops.supervised_flow_loss(fl, maps, q=0.4),
        "selfsup": lambda fl: ops.selfsup_flow_loss(fl[0][:1], *pair, 0.4) + 0.0 * fl[1].sum(),
        "smooth": lambda fl: ops.flow_smoothness(batch, fl, 10.0, order=2),
    }
    want, gw = 0.0, [torch.zeros_like(g, dtype=torch.float64) for g in gb]
    for name, fn in alone.items():
        v, g, _ = grads(fn)
        assert v > 0 and all(gk.abs().max() > 0 for gk in g[:1 if name == "selfsup" else 2]), name
        want += SIX_W[name] * v
        for k in range(2):
            gw[k] += SIX_W[name] * g[k].double()
    errs = [rel_l2(gb[k], gw[k]) for k in range(2)]
    print("six terms: loss", both, want, "d(flow) rel_l2", errs)
    assert abs(both - want) <= REL_TOL * abs(want)
    assert all(e < REL_TOL for e in errs), errs
    routed, gr, fgs = grads(lambda fl: _six(ops, batch, fl, maps, pair), attach=True)
    try:
        assert routed == both
        for g, p, fg in zip(gr, gb, fgs):
            assert fg.filled
            assert torch.equal(g, p)
    finally:
        for fg in fgs:
            fg.release()


# --------------------------------------------------------------------- saved tensors ----
def _all_six(ops, b, f):
    """The first two levels: four photometric groups plus five would be nine sum groups."""
    maps, pair = _labels()
    return ops.census_flow_loss(b, f[:2], 0.5, 3, 0.5, 0.2, 10, convention="image",
                                ssim_weight=0.3, supervised_weight=0.7, gt=maps,
                                selfsup_weight=0.5, selfsup=pair)


# id: (call, what loss.grad_fn.saved_tensors holds)
SAVED = {
    "photometric": (ROWS["photometric"][0], dict(pyramid=LEVELS, flows=LEVELS)),
    "census": (ROWS["census"][0], dict(planes=LEVELS)),
    "ssim": (ROWS["ssim"][0], dict(planes=LEVELS)),
    "supervised": (ROWS["supervised"][0], dict(planes=LEVELS)),
    "selfsup": (ROWS["selfsup"][0], dict(planes=1)),
    "smoothness_alpha0": (ROWS["smoothness_alpha0"][0], dict(flows=LEVELS)),
    "smoothness_alpha10": (ROWS["smoothness_alpha10"][0], dict(pyramid=LEVELS, flows=LEVELS)),
    "census_smoothness_alpha0": (
        lambda ops, b, f: ops.census_flow_loss(b, f, 0.5, 3, 0.0, 0.2, 0.0),
        dict(flows=LEVELS, planes=LEVELS)),
    "six_terms": (_all_six, dict(pyramid=2, flows=2, planes=3 * 2 + 1)),
}


# where a forward entry takes its plane pointer(s), counted from the end (the stream is last)
PLANES_ARG = {"of_census_fwd_multi": -3, "of_census_fwd_multi_cv": -4, "of_census_fwd_multi_w": -4,
              "of_ssim_fwd_multi": -4, "of_supervised_fwd_multi": -3, "of_flow_distill_fwd": -3}


def _spy_planes(monkeypatch, ops):
    """Per forward entry that can write planes: whether it was asked to."""
    asked = []
    real = ops.call

    def call(name, *a):
        if name in PLANES_ARG:
            asked.append(a[PLANES_ARG[name]] is not None)
        return real(name, *a)
    monkeypatch.setattr(ops, "call", call)
    return asked


@pytest.mark.parametrize("row", list(SAVED))
def test_saved_tensors(monkeypatch, row):
    """What the forward keeps for the backward (the comment in _Loss.forward): the pyramid for
    the photometric term and edge-weighted smoothness, the flows for those two terms, and for
    census, SSIM, the supervised and the self-supervision term only their planes, in that
    order.  With no flow requiring grad there is no graph, and no forward entry is handed a
    plane to write (with one, every plane-writing entry is)."""
    from optical_flow_amd import ops
    fn, want = SAVED[row]
    batch, flows = _inputs()
    asked = _spy_planes(monkeypatch, ops)
    fd = [dev(f).requires_grad_(True) for f in flows]
    loss = fn(ops, batch, fd)
    assert all(asked) and bool(asked) == ("planes" in want)
    n_entries = len(asked)
    del asked[:]
    saved = list(loss.grad_fn.saved_tensors)
    np_, nf = want.get("pyramid", 0), want.get("flows", 0)
    assert len(saved) == np_ + nf + want.get("planes", 0)
    for k, t in enumerate(saved[:np_]):
        assert t.shape == (N, S >> (k + 1), S >> (k + 1), 6)
    for t, f in zip(saved[np_:np_ + nf], fd):
        assert t.data_ptr() == f.data_ptr()
    known = {f.data_ptr() for f in fd} | {t.data_ptr() for t in saved[:np_]}
    for t in saved[np_ + nf:]:
        assert t.shape[-1] == 2 and t.data_ptr() not in known
    fd = [dev(f) for f in flows]
    assert fn(ops, batch, fd).grad_fn is None
    assert len(asked) == n_entries and not any(asked)
