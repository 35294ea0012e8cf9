"""Occlusion masks, host side (DESIGN.md "Occlusion masks"): argument checks of LossLayer,
ops.occlusion_masks and the train command, the step log's header, LossLayer's dispatch, the
float64 reference's own consistency (tests/occlusion_ref.py), the known answer on shifted
pairs, and the conditioning of the inputs that tests/test_gpu_occlusion.py compares on."""
import pytest
import torch

import census_ref
import occlusion_ref as O
from helpers import f64, rng_tensor
from oracle import ref_flow as R
from warp_image_ref import image_convention, shifted_pair, true_flows


# ---------------------------------------------------------------------- argument checks ----
def test_loss_layer_argument_checks():
    from optical_flow_amd.loss import LossLayer
    for kw in (dict(occlusion="forward"), dict(occlusion=None),
               dict(occlusion="fb", occlusion_alpha1=-0.1),
               dict(occlusion="border", occlusion_alpha2=-1.0),
               dict(occlusion_alpha1=float("nan"))):
        with pytest.raises(ValueError):
            LossLayer(warp_convention="image", **kw)
    for mode in ("border", "fb"):
        with pytest.raises(ValueError, match="image"):
            LossLayer(occlusion=mode)                       # the reference convention
        with pytest.raises(ValueError, match="image"):
            LossLayer(occlusion=mode, warp_convention="reference")
    layer = LossLayer(warp_convention="image", occlusion="fb", occlusion_alpha1=0.02,
                      occlusion_alpha2=0.25)
    assert (layer.occlusion, layer.occlusion_alpha1, layer.occlusion_alpha2) == ("fb", 0.02, 0.25)
    d = LossLayer()
    assert (d.occlusion, d.occlusion_alpha1, d.occlusion_alpha2) == ("none", 0.01, 0.5)


def test_fb_needs_the_doubled_batch():
    """An odd batch cannot be [pairs ; swapped pairs]: ValueError from the layer and from
    ops.occlusion_masks, before any kernel."""
    from optical_flow_amd import ops
    from optical_flow_amd.loss import LossLayer
    batch = torch.zeros(3, 16, 16, 6)
    flows = [torch.zeros(3, 8, 8, 2), torch.zeros(3, 4, 4, 2)]
    with pytest.raises(ValueError, match="even"):
        LossLayer(warp_convention="image", occlusion="fb")(batch, flows)
    with pytest.raises(ValueError, match="even"):
        ops.occlusion_masks(flows, "fb")


def test_occlusion_masks_argument_checks():
    from optical_flow_amd import ops
    flows = [torch.zeros(2, 8, 8, 2)]
    with pytest.raises(ValueError, match="mode"):
        ops.occlusion_masks(flows, "none")
    with pytest.raises(ValueError, match="image"):
        ops.occlusion_masks(flows, "border", convention="reference")
    with pytest.raises(ValueError):
        ops.occlusion_masks(flows, "border", convention="xy")
    with pytest.raises(ValueError, match="alpha"):
        ops.occlusion_masks(flows, "fb", alpha1=-1e-3)
    with pytest.raises(ValueError, match="alpha"):
        ops.occlusion_masks(flows, "fb", alpha2=-0.5)


def test_train_command_arguments():
    from optical_flow_amd.train import build_parser, check_occlusion_args, header_record, main
    ap = build_parser()
    args = ap.parse_args([])
    assert (args.occlusion, args.occ_alpha1, args.occ_alpha2) == ("none", 0.01, 0.5)
    check_occlusion_args(args)
    assert header_record(args) is None                          # a default run: no header
    for mode in ("border", "fb"):
        with pytest.raises(ValueError, match="--warp-convention image"):
            check_occlusion_args(ap.parse_args(["--occlusion", mode]))
        check_occlusion_args(ap.parse_args(["--occlusion", mode, "--warp-convention", "image"]))
    with pytest.raises(ValueError, match="alpha"):
        check_occlusion_args(ap.parse_args(["--occ-alpha1", "-0.5"]))
    with pytest.raises(ValueError, match="alpha"):
        check_occlusion_args(ap.parse_args(["--occ-alpha2", "-0.5"]))
    with pytest.raises(SystemExit):
        ap.parse_args(["--occlusion", "both"])
    with pytest.raises(SystemExit):                             # main: a parser error
        main(["--occlusion", "fb"])
    head = header_record(ap.parse_args(["--occlusion", "fb", "--occ-alpha1", "0.02",
                                        "--occ-alpha2", "0.25", "--warp-convention", "image"]))
    assert (head["occlusion"], head["occ_alpha1"], head["occ_alpha2"]) == ("fb", 0.02, 0.25)
    assert head["header"] is True and head["warp_convention"] == "image"
    head = header_record(ap.parse_args(["--occlusion", "border", "--warp-convention", "image"]))
    assert (head["occlusion"], head["occ_alpha1"], head["occ_alpha2"]) == ("border", 0.01, 0.5)
    assert "occlusion" not in header_record(ap.parse_args(["--warp-convention", "image"]))


# ----------------------------------------------------------------------------- dispatch ----
def _record_ops(monkeypatch):
    from optical_flow_amd import ops
    calls = []

    def rec(name, ret):
        def f(*a, **kw):
            calls.append((name, a, kw))
            return ret
        monkeypatch.setattr(ops, name, f)
    for name in ("photometric_loss", "flow_loss", "census_flow_loss"):
        rec(name, name)
    rec("occlusion_masks", ["m0", "m1"])
    return calls


def test_default_dispatch_is_unchanged(monkeypatch):
    """occlusion="none" (the default): LossLayer calls exactly the ops function, with exactly
    the arguments, it called before the argument existed; ops.occlusion_masks is not called."""
    from optical_flow_amd.loss import LossLayer
    calls = _record_ops(monkeypatch)
    batch = torch.zeros(2, 16, 16, 6)
    flows = [torch.zeros(2, 8, 8, 2), torch.zeros(2, 4, 4, 2)]
    for kw in ({}, {"occlusion": "none"}):
        for cv in ("reference", "image"):
            del calls[:]
            assert LossLayer(warp_convention=cv, **kw)(batch, flows) == "photometric_loss"
            assert LossLayer(0.2, 10, warp_convention=cv, **kw)(batch, flows) == "flow_loss"
            assert LossLayer(0.2, 10, census_weight=0.5, census_radius=2, photometric_weight=0.25,
                             warp_convention=cv, **kw)(batch, flows) == "census_flow_loss"
            assert [c[0] for c in calls] == ["photometric_loss", "flow_loss", "census_flow_loss"]
            assert calls[0][1][2:] == (cv,) and calls[0][2] == {}
            assert calls[1][1][2:] == (0.2, 10.0, 1e-4, cv) and calls[1][2] == {}
            assert calls[2][1][2:] == (0.5, 2, 0.25, 0.2, 10.0, 1e-4, cv) and calls[2][2] == {}
            for c in calls:
                assert c[1][0] is batch and all(a is b for a, b in zip(c[1][1], flows))


@pytest.mark.parametrize("mode", ["border", "fb"])
def test_occlusion_dispatch(monkeypatch, mode):
    """With a mode every legal weight combination goes through ops.census_flow_loss with the
    masks of the detached flows; the alphas and the convention reach ops.occlusion_masks."""
    from optical_flow_amd.loss import LossLayer
    calls = _record_ops(monkeypatch)
    batch = torch.zeros(2, 16, 16, 6)
    flows = [torch.zeros(2, 8, 8, 2, requires_grad=True), torch.zeros(2, 4, 4, 2)]
    for args, kw, want in (((), {}, (0.0, 3, 1.0, 0.0, 0.0, 1e-4)),
                           ((0.2, 10), {}, (0.0, 3, 1.0, 0.2, 10.0, 1e-4)),
                           ((0.2, 10), dict(census_weight=0.5, photometric_weight=0.0),
                            (0.5, 3, 0.0, 0.2, 10.0, 1e-4))):
        del calls[:]
        layer = LossLayer(*args, warp_convention="image", occlusion=mode, occlusion_alpha1=0.02,
                          occlusion_alpha2=0.25, **kw)
        assert layer(batch, flows) == "census_flow_loss"
        assert [c[0] for c in calls] == ["occlusion_masks", "census_flow_loss"]
        (_, ma, mk), (_, la, lk) = calls
        assert ma[1:] == (mode, 0.02, 0.25, "image") and mk == {}
        assert not any(f.requires_grad for f in ma[0])
        assert la[2:] == want + ("image",) and lk == {"weights": ["m0", "m1"]}


def test_trainer_doubles_the_batch_for_fb():
    """Trainer.train_step with a loss layer whose occlusion is "fb" runs the net and the loss
    on [batch ; batch with the two images exchanged] and returns the first B images of every
    flow level; any other layer (or one without the attribute) sees the batch as passed."""
    import types
    from optical_flow_amd.train import Trainer
    seen = {}

    class Net:
        store = types.SimpleNamespace(zero_grad=lambda: None)

        def __call__(self, b):
            seen["net"] = b
            self.p = torch.zeros((), requires_grad=True)
            return [self.p + torch.arange(b.shape[0] * 4.0).reshape(b.shape[0], 2, 2, 1)]

    class Loss:
        def __init__(self, occ):
            if occ is not None:
                self.occlusion = occ

        def __call__(self, b, flows):
            seen["loss"] = b
            return flows[0].sum()

    batch = torch.arange(2 * 4 * 4 * 6.0).reshape(2, 4, 4, 6)
    opt = types.SimpleNamespace(apply_gradients=lambda grad_scale: None)
    for occ, n in ((None, 2), ("none", 2), ("border", 2), ("fb", 4)):
        tr = Trainer(Net(), opt, Loss(occ), data_parallel=False)
        loss, flows = tr.train_step(batch)
        assert seen["net"] is seen["loss"] and seen["net"].shape[0] == n
        assert torch.equal(seen["net"][:2], batch)
        if occ == "fb":
            assert torch.equal(seen["net"][2:, ..., :3], batch[..., 3:])
            assert torch.equal(seen["net"][2:, ..., 3:], batch[..., :3])
        assert flows[0].shape[0] == 2 and not flows[0].requires_grad
        assert torch.equal(flows[0], torch.arange(8.0).reshape(2, 2, 2, 1))


# -------------------------------------------------------------- the reference's own checks ----
def _level(h, w, seed):
    img = f64(rng_tensor((2, h, w, 6), seed, lo=-0.5, hi=0.6))
    flow = f64(rng_tensor((2, h, w, 2), seed + 1, scale=1.5))
    wt = f64(rng_tensor((2, h, w), seed + 2, lo=0.0, hi=1.0))
    return img, flow, wt


def test_unit_weights_reproduce_the_unweighted_references():
    img, flow, _ = _level(9, 11, 7)
    g1, u = O.gray_pair(img, flow)
    ones = torch.ones_like(g1)
    for r in (1, 2, 3):
        a, b = O.census_level(g1, u, ones, r).item(), census_ref.level_sum(g1, u, r).item()
        assert abs(a - b) <= 1e-12 * abs(b)
    batch = f64(rng_tensor((2, 32, 48, 6), 3, lo=-0.5, hi=0.6))
    flows = [f64(rng_tensor((2, 32 >> (s + 1), 48 >> (s + 1), 2), 60 + s, scale=1.5))
             for s in range(3)]
    ones = [torch.ones(f.shape[:3], dtype=torch.float64) for f in flows]
    with image_convention():
        want_p = R.photometric_loss(batch, flows).item()
        want_c = census_ref.census(batch, flows, 2).item()
    for wts in (None, ones):
        assert abs(O.photometric(batch, flows, wts).item() - want_p) <= 1e-12 * want_p
        assert abs(O.census(batch, flows, 2, wts).item() - want_c) <= 1e-12 * want_c


@pytest.mark.parametrize("r", [1, 2, 3])
def test_weighted_closed_form_is_the_gradient_of_the_definition(r):
    """dC/du[q] = (1/K) sum_o (w[q] + w[q+o]) phi'(e[q,o]) tau'(u[q+o] - u[q]) (what the kernel
    gathers) equals autograd of the definition, to 1e-10, on a 9 x 11 level."""
    img, flow, wt = _level(9, 11, 11)
    g1, u = O.gray_pair(img, flow)
    u = u.clone().requires_grad_(True)
    c = O.census_level(g1, u, wt, r)
    grad = torch.autograd.grad(c, u)[0]
    c2, grad2 = O.census_level_closed_form(g1, u.detach(), wt, r)
    assert abs(c.item() - c2.item()) <= 1e-12 * abs(c.item())
    err = (grad - grad2).abs().max().item()
    print("r", r, "max |closed form - autograd|", err, "of", grad.abs().max().item())
    assert grad.abs().max().item() > 1e-6 and err < 1e-10


@pytest.mark.parametrize("dx,dy,share", [(16, -16, 0.625), (-32, 16, 0.5)])
def test_known_answer_on_shifted_pairs(dx, dy, share):
    """A pure translation scored with its true flow: every error comes from the pixels whose
    sample lies outside the frame.  Border-masked photometric mean of every level < 1e-12,
    unmasked > 0.05, valid share (64 - |dy|)(96 - |dx|) / (64 * 96)."""
    pair, flows = shifted_pair(64, 96, dx, dy), true_flows(64, 96, dx, dy)
    masks = O.masks(flows, "border")
    for s, (f, m) in enumerate(zip(flows, masks)):
        n, h, w, _ = f.shape
        r = R.resize_bilinear(pair, h, w)
        masked = O.photo_level(r, f, m).item() / (n * h * w * 3)
        plain = O.photo_level(r, f).item() / (n * h * w * 3)
        print("level", s, "masked", masked, "unmasked", plain, "valid", m.mean().item())
        assert masked < 1e-12 and plain > 0.05
        assert m.mean().item() == share
    assert O.photometric(pair, flows, masks).item() < 1e-12
    assert O.photometric(pair, flows).item() > 0.05


# ------------------------------------------------ conditioning of the GPU tests' inputs ----
@pytest.mark.parametrize("mode", ["border", "fb"])
def test_abi_inputs_are_well_conditioned(mode):
    """The mask kernel is compared on every pixel that is not near a decision: near pixels are
    at most 1 % of each level, and on every level of at least 13 x 21 pixels each mask value
    covers at least 10 %."""
    for l, f in enumerate(O.abi_flows(mode)):
        f = f64(f)
        a2 = O.ABI_ALPHA2S[l]
        m = O.border(f)[0] if mode == "border" else O.fb(f, O.ABI_ALPHA1, a2)[0]
        nr = O.near(f, mode, O.ABI_ALPHA1, a2).double().mean().item()
        valid = m.mean().item()
        print(mode, tuple(f.shape), "valid %.4f near %.5f" % (valid, nr))
        assert nr <= 0.01
        if f.shape[1] >= 13 and f.shape[2] >= 21:
            assert 0.1 <= valid <= 0.9


@pytest.mark.parametrize("mode", ["border", "fb"])
def test_loss_parity_inputs_have_no_near_pixels(mode):
    """The LossLayer parity case: no pixel within 1e-3 of a decision (one flipped mask pixel
    would move the loss), and both mask values on >= 10 % of every level of >= 13 x 21."""
    batch, flows = O.layer_case(mode)
    assert batch.shape[0] == O.LAYER_SIZE[mode][0] and len(flows) == 4
    if mode == "fb":
        b = batch.shape[0] // 2
        assert torch.equal(batch[b:, ..., :3], batch[:b, ..., 3:])
        assert torch.equal(batch[b:, ..., 3:], batch[:b, ..., :3])
    for s, f in enumerate(flows):
        assert f.dtype == torch.float32
        f = f64(f)
        a2 = 0.5 / 4.0 ** (s + 1)
        assert not O.near(f, mode, 0.01, a2, tol=1e-3).any()
        m = O.masks([f], mode, 0.01, 0.5 * 4.0 ** -s)[0]
        assert torch.equal(m, O.border(f)[0] if mode == "border" else O.fb(f, 0.01, a2)[0])
        valid = m.mean().item()
        print(mode, tuple(f.shape), "valid %.4f" % valid)
        if f.shape[1] >= 13 and f.shape[2] >= 21:
            assert 0.1 <= valid <= 0.9
