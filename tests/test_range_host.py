"""Range-map occlusion, host side (DESIGN.md "Range-map occlusion"): on the float64 reference
alone (tests/range_ref.py) the conditions that tests/test_gpu_range.py relies on -- the cap on
taps per pixel behind its tolerance, no pixel near a border decision, both clamp regimes well
represented -- the reference's known answers, and the argument checks and the dispatch of
LossLayer, ops, Trainer and the train command that need no GPU."""
import types

import pytest
import torch

import range_ref as RR
from helpers import f64

MAX_TAPS = 32               # the cap test_gpu_range.py's absolute tolerance is derived from


# ------------------------------------------------ conditioning of the GPU tests' inputs ----
@pytest.mark.parametrize("scale", [0.3, 1.0, 3.0])
def test_at_most_32_taps_land_on_a_pixel(scale):
    worst = max(int(RR.tap_counts(f64(f)).max()) for f in RR.abi_flows(scale))
    print("scale", scale, "most taps on one pixel", worst)
    assert 1 <= worst <= MAX_TAPS


def test_abi_inputs_are_well_conditioned():
    """No pixel within 1e-4 of a border decision; on the two larger levels R < 1 on >= 10 %,
    mask == 1 on >= 10 % and mask == 0 on >= 2 % of the pixels."""
    for f in RR.abi_flows():
        f = f64(f)
        assert not RR.near(f, "border").any()
        R, m = RR.range_map(f), RR.mask(f)
        assert (R >= 0).all() and (m >= 0).all() and (m <= 1).all()
        soft, one, zero = [(v.double().mean().item()) for v in (R < 1, m == 1, m == 0)]
        print(tuple(f.shape), "R<1 %.3f mask==1 %.3f mask==0 %.3f" % (soft, one, zero))
        if f.shape[1] >= 13 and f.shape[2] >= 21:
            assert soft >= 0.10 and one >= 0.10 and zero >= 0.02


def test_layer_case_has_no_near_pixels():
    batch, flows = RR.layer_case()
    assert tuple(batch.shape) == (4, 48, 80, 6) and len(flows) == 4
    assert torch.equal(batch[2:, ..., :3], batch[:2, ..., 3:])
    for s, f in enumerate(flows):
        assert f.dtype == torch.float32 and tuple(f.shape) == (4, 48 >> (s + 1), 80 >> (s + 1), 2)
        assert not RR.near(f64(f), "border", tol=1e-3).any()
        m = RR.mask(f64(f))
        print(tuple(f.shape), "mean weight %.3f" % m.mean().item())
        if f.shape[1] >= 12:
            assert 0.1 <= m.mean().item() <= 0.9


# ------------------------------------------------------------------------ known answers ----
H, W, B = 13, 21, 2


def test_zero_flows_give_one():
    f = f64(RR.known_flows(H, W)["zero"])
    assert (RR.range_map(f) == 1.0).all() and (RR.mask(f) == 1.0).all()


def test_integer_translation_gives_the_border_mask():
    """Forward (+2, 0), backward (-2, 0): min(1, R) is the border mask itself, zero in columns
    w-2, w-1 of the forward images and in columns 0, 1 of the swapped ones."""
    f = f64(RR.known_flows(H, W)["shift"])
    want = torch.ones(2 * B, H, W, dtype=torch.float64)
    want[:B, :, W - 2:] = 0.0
    want[B:, :, :2] = 0.0
    assert torch.equal(RR.border(f)[0], want)
    assert torch.equal(RR.range_map(f).clamp(max=1.0), want)
    assert torch.equal(RR.mask(f), want)


def test_contraction():
    """Backward flow -q/2 (the points q/2): per axis the sources 2p-1, 2p, 2p+1 weigh 0.5, 1,
    0.5 on p, so R = 4 where all of them exist, 1.5^2 at the corner (0, 0), 0 at the far one."""
    R = RR.range_map(f64(RR.known_flows(H, W)["contract"]))
    assert (R[:B, 1:(H - 2) // 2 + 1, 1:(W - 2) // 2 + 1] == 4.0).all()
    assert (R[:B, 0, 0] == 2.25).all() and (R[:B, H - 1, W - 1] == 0.0).all()
    assert (R[B:] == 1.0).all()                         # the forward flows are zero


def test_expansion():
    """Backward flow +q (the points 2q): R = 1 where both coordinates are even, 0 elsewhere."""
    R = RR.range_map(f64(RR.known_flows(H, W)["expand"]))
    want = torch.zeros(H, W, dtype=torch.float64)
    want[0::2, 0::2] = 1.0
    assert all(torch.equal(R[b], want) for b in range(B))


def test_non_finite_and_far_sources_are_dropped():
    bad, clean, keep = RR.edge_flows()
    assert (~torch.isfinite(bad)).sum() == 4 and (bad.abs() == 1e9).sum() == 4
    assert (~keep).sum() == 8
    R = RR.range_map(f64(bad))
    assert torch.isfinite(R).all() and torch.isfinite(RR.mask(f64(bad))).all()
    assert torch.equal(R, RR.range_map(f64(clean), keep))
    assert not torch.equal(R, RR.range_map(f64(clean)))


def test_partner_is_the_other_half():
    f = f64(RR.abi_flows()[2])
    other = torch.cat([f[:B], f[B:].flip(0)], 0)
    assert torch.equal(RR.range_map(other)[:B], RR.range_map(f)[:B].flip(0))


# ---------------------------------------------------------------------- argument checks ----
def test_loss_layer_argument_checks():
    from optical_flow_amd.loss import LossLayer
    with pytest.raises(ValueError, match="image"):
        LossLayer(occlusion="range")
    with pytest.raises(ValueError, match="image"):
        LossLayer(occlusion="range", warp_convention="reference")
    with pytest.raises(ValueError, match="'range'"):
        LossLayer(occlusion="wang", warp_convention="image")
    layer = LossLayer(warp_convention="image", occlusion="range")
    assert layer.occlusion == "range"
    batch = torch.zeros(3, 16, 16, 6)
    flows = [torch.zeros(3, 8, 8, 2), torch.zeros(3, 4, 4, 2)]
    with pytest.raises(ValueError, match="even"):
        layer(batch, flows)


def test_ops_argument_checks():
    from optical_flow_amd import _lib, ops
    assert _lib.OCC_RANGE == 3
    assert ops.OCCLUSION_MODES == {"border": 1, "fb": 2, "range": 3}
    assert [ops.needs_swapped_pairs(m) for m in ("none", "border", "fb", "range")] == \
        [False, False, True, True]
    with pytest.raises(ValueError, match="range"):
        ops.occlusion_masks([torch.zeros(2, 8, 8, 2)], "wang")
    for n in (3, 1, 0):
        flows = [torch.zeros(n, 8, 8, 2)]
        with pytest.raises(ValueError, match="even"):
            ops.occlusion_masks(flows, "range")
        with pytest.raises(ValueError, match="even"):
            ops.range_map(flows)
    with pytest.raises(ValueError, match="image"):
        ops.occlusion_masks([torch.zeros(2, 8, 8, 2)], "range", convention="reference")
    with pytest.raises(ValueError, match="levels"):
        ops.range_map([torch.zeros(2, 8, 8, 2)] * 9)


def test_train_command_arguments():
    from optical_flow_amd.train import build_parser, check_occlusion_args, header_record, main
    ap = build_parser()
    with pytest.raises(ValueError, match="--warp-convention image"):
        check_occlusion_args(ap.parse_args(["--occlusion", "range"]))
    args = ap.parse_args(["--occlusion", "range", "--warp-convention", "image"])
    check_occlusion_args(args)
    head = header_record(args)
    assert head["occlusion"] == "range" and head["warp_convention"] == "image"
    with pytest.raises(SystemExit):                             # main: a parser error
        main(["--occlusion", "range"])


# ----------------------------------------------------------------------------- dispatch ----
def test_range_dispatch(monkeypatch):
    """LossLayer(occlusion="range") goes where "fb" goes: ops.occlusion_masks on the detached
    flows, then ops.census_flow_loss with the masks as weights."""
    from optical_flow_amd import ops
    from optical_flow_amd.loss import LossLayer
    calls = []
    monkeypatch.setattr(ops, "occlusion_masks",
                        lambda *a, **kw: calls.append(("masks", a, kw)) or ["m0", "m1"])
    monkeypatch.setattr(ops, "census_flow_loss",
                        lambda *a, **kw: calls.append(("loss", a, kw)) or "loss")
    monkeypatch.setattr(ops, "_gt_handle", lambda gt, n: ("gt", n))
    batch = torch.zeros(4, 16, 16, 6)
    flows = [torch.zeros(4, 8, 8, 2, requires_grad=True), torch.zeros(4, 4, 4, 2)]
    layer = LossLayer(0.2, 10, census_weight=0.5, photometric_weight=0.0,
                      warp_convention="image", occlusion="range")
    assert layer(batch, flows) == "loss"
    (_, ma, mk), (_, la, lk) = calls
    assert ma[1:] == ("range", 0.01, 0.5, "image") and mk == {}
    assert not any(f.requires_grad for f in ma[0])
    assert la[2:] == (0.5, 3, 0.0, 0.2, 10.0, 1e-4, "image") and lk == {"weights": ["m0", "m1"]}
    assert layer._forward_gt("x", 4) == ("gt", 2)       # the truth of the forward half


def test_trainer_doubles_the_batch_for_range():
    from optical_flow_amd.train import Trainer
    seen = {}

    class Net:
        store = types.SimpleNamespace(zero_grad=lambda: None)

        def __call__(self, b):
            seen["net"] = b
            self.p = torch.zeros((), requires_grad=True)
            return [self.p + torch.arange(b.shape[0] * 4.0).reshape(b.shape[0], 2, 2, 1)]

    class Loss:
        occlusion = "range"

        def __call__(self, b, flows):
            seen["loss"] = b
            return flows[0].sum()

    batch = torch.arange(2 * 4 * 4 * 6.0).reshape(2, 4, 4, 6)
    opt = types.SimpleNamespace(apply_gradients=lambda grad_scale: None)
    tr = Trainer(Net(), opt, Loss(), data_parallel=False)
    _, flows = tr.train_step(batch)
    assert seen["net"] is seen["loss"] and seen["net"].shape[0] == 4
    assert torch.equal(seen["net"][:2], batch)
    assert torch.equal(seen["net"][2:, ..., :3], batch[..., 3:])
    assert torch.equal(seen["net"][2:, ..., 3:], batch[..., :3])
    assert torch.equal(flows[0], torch.arange(8.0).reshape(2, 2, 2, 1))
