"""The loss's launch sequences and its FlowGrad protocol (DESIGN.md "The loss Function"): which
C entry points each public loss entry calls, in which order and with which ``accumulate``, for
every combination of terms; that the entries of the training loss write a flow head's gradient
buffer and the two stand-alone terms never do; and the seven-level census + smoothness loss.

Shapes: n = 2, a 32 x 32 batch and four flows of 16 x 16 down to 2 x 2, the smallest at which
every branch exists (a level smaller than the census window, one with a single pair per
direction)."""
import functools

import pytest
import torch

from helpers import dev, rel_l2, rng_tensor

pytestmark = pytest.mark.gpu

N, S, LEVELS = 2, 32, 4
BWD_WITH_ACC = ("of_census_bwd_multi", "of_flow_smooth_bwd_multi")


@functools.lru_cache(maxsize=None)
def _inputs(n=N, size=S, levels=LEVELS):
    from optical_flow_amd.data import synthetic_batch
    batch = dev(torch.from_numpy(synthetic_batch(n, size, size, seed=5)))
    flows = [rng_tensor((n, size >> (s + 1), size >> (s + 1), 2), 50 + s, scale=2.0)
             for s in range(levels)]
    return batch, flows


def _ones(flows):
    return [torch.ones(f.shape[:3], device="cuda") for f in flows]


def _three(ops, b, f, **kw):
    return ops.census_flow_loss(b, f, 0.5, 3, 0.5, 0.2, 10, **kw)


PYR, SUM = "of_pyramid6", "of_sum_partials"
PF, PB = "of_photo_l1_fwd_multi", "of_photo_l1_bwd_multi"
CF, SF = "of_census_fwd_multi", "of_flow_smooth_fwd_multi"
CB0, CB1 = "of_census_bwd_multi(acc 0)", "of_census_bwd_multi(acc 1)"
SB0, SB1 = "of_flow_smooth_bwd_multi(acc 0)", "of_flow_smooth_bwd_multi(acc 1)"

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
}


def _spy(monkeypatch, ops):
    called = []
    real = ops.call

    def call(name, *a):
        # accumulate is the argument before the stream
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
