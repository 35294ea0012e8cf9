"""The image-coordinate warp convention, host side: the known-answer property that motivates
it (the true flow brings the photometric residual to zero in the image convention and cannot
in the reference's transposed one), the argument validation of every layer that takes the
convention, the _cv entry points' refusal of an unknown code, and the step log's header."""
import ctypes as C
import os
import types

import pytest
import torch

from oracle import ref_flow as R
from warp_image_ref import (image_convention, interior_residuals, shifted_pair, true_flows,
                            warp_features_image)

H, W, DX, DY = 64, 96, 16, -16


@pytest.fixture(scope="module")
def lib():
    from optical_flow_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def test_zero_flow_is_identity_in_image_convention():
    f2 = torch.rand((2, 5, 9, 3), dtype=torch.float64)
    z = torch.zeros((2, 5, 9, 2), dtype=torch.float64)
    assert torch.equal(warp_features_image(z, f2), f2)
    assert not torch.equal(R.warp_features(z, f2), f2)       # a transpose-and-clamp


def test_true_flow_zeroes_the_residual_only_in_image_convention():
    """A 64 x 96 pair, image 2 = image 1 shifted by (dx, dy) = (16, -16), edge-replicated; the
    true constant flow (-dx, -dy) / 2^(s+1) at all four scales.  Interior = at least
    |shift| / 2^(s+1) from each border.  Image convention: every interior pixel's residual is
    <= 1e-12 in float64.  Reference convention: the interior residual stays > 0.1 with the
    true flow, the component-swapped flow and zero flow."""
    pair = shifted_pair(H, W, DX, DY)
    flows = true_flows(H, W, DX, DY)
    with image_convention():
        res = interior_residuals(pair, flows, DX, DY)
        assert R.photometric_loss(pair, flows).item() < 0.2       # (the borders only)
    print("image convention, interior residual per scale:", res)
    assert all(r <= 1e-12 for r in res), res
    swapped = [f.flip(-1) for f in flows]
    zero = [torch.zeros_like(f) for f in flows]
    for name, fl in (("true", flows), ("swapped", swapped), ("zero", zero)):
        res = interior_residuals(pair, fl, DX, DY)
        print("reference convention, %s flow, interior residual per scale:" % name, res)
        assert all(r > 0.1 for r in res), (name, res)


def test_patch_is_undone():
    orig = R.warp_features
    with image_convention():
        assert R.warp_features is warp_features_image
    assert R.warp_features is orig


# ---------------------------------------------------------------- validation ------------
def test_bad_names_raise_value_error():
    from optical_flow_amd import ops
    from optical_flow_amd.loss import LossLayer
    from optical_flow_amd.model import FlowNet, build_flow_net, flow_module, warp_features
    from optical_flow_amd.train import build_parser
    t, f = torch.zeros(1, 4, 4, 8), torch.zeros(1, 4, 4, 2)
    for bad in ("Image", "transposed", "", None, 1):
        with pytest.raises(ValueError, match="warp convention"):
            ops.warp_convention(bad)
        with pytest.raises(ValueError, match="warp convention"):
            ops.warp(t, f, convention=bad)
        with pytest.raises(ValueError, match="warp convention"):
            warp_features(f, t, convention=bad)
        with pytest.raises(ValueError, match="warp convention"):
            flow_module(t, t, None, 3, head=object(), convention=bad)
        with pytest.raises(ValueError, match="warp convention"):
            FlowNet(64, 128, warp_convention=bad)
        with pytest.raises(ValueError, match="warp convention"):
            build_flow_net(64, 128, warp_convention=bad)
        with pytest.raises(ValueError, match="warp convention"):
            LossLayer(warp_convention=bad)
        for fn in (ops.photometric_loss, ops.census_loss):
            with pytest.raises(ValueError, match="warp convention"):
                fn(torch.zeros(1, 8, 8, 6), [torch.zeros(1, 4, 4, 2)], convention=bad)
        with pytest.raises(ValueError, match="warp convention"):
            ops.flow_loss(torch.zeros(1, 8, 8, 6), [torch.zeros(1, 4, 4, 2)], 0.1, convention=bad)
        with pytest.raises(ValueError, match="warp convention"):
            ops.census_flow_loss(torch.zeros(1, 8, 8, 6), [torch.zeros(1, 4, 4, 2)], 0.1,
                                 convention=bad)
    assert ops.warp_convention("reference") == 0 and ops.warp_convention("image") == 1
    assert LossLayer().warp_convention == "reference"
    assert LossLayer(warp_convention="image").warp_convention == "image"
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--warp-convention", "transposed"])
    assert build_parser().parse_args([]).warp_convention == "reference"


def test_trainer_refuses_a_mismatch():
    from optical_flow_amd.loss import LossLayer
    from optical_flow_amd.train import Trainer, check_warp_conventions
    net_r = types.SimpleNamespace(warp_convention="reference", store=None)
    net_i = types.SimpleNamespace(warp_convention="image", store=None)
    plain = types.SimpleNamespace(store=None)                     # (TwoLayerHead: no attribute)
    assert check_warp_conventions(net_r, LossLayer()) == "reference"
    assert check_warp_conventions(net_i, LossLayer(warp_convention="image")) == "image"
    assert check_warp_conventions(plain, LossLayer()) == "reference"
    for net, loss in ((net_r, LossLayer(warp_convention="image")), (net_i, LossLayer()),
                      (plain, LossLayer(warp_convention="image"))):
        with pytest.raises(ValueError, match="convention"):
            check_warp_conventions(net, loss)
        with pytest.raises(ValueError, match="convention"):
            Trainer(net, optimizer=object(), loss_layer=loss, data_parallel=False)
    # without a loss layer the trainer builds one in the net's convention
    tr = Trainer(net_i, optimizer=object(), data_parallel=False)
    assert tr.loss_layer.warp_convention == "image"
    assert Trainer(net_r, optimizer=object(), data_parallel=False).loss_layer.warp_convention \
        == "reference"


def test_header_record_carries_the_convention():
    from optical_flow_amd.train import build_parser, header_record
    ap = build_parser()
    assert header_record(ap.parse_args([])) is None               # a default run: no header
    assert header_record(ap.parse_args(["--warp-convention", "reference"])) is None
    head = header_record(ap.parse_args(["--warp-convention", "image"]))
    assert head["header"] is True and head["warp_convention"] == "image"
    assert "step" not in head
    head = header_record(ap.parse_args(["--smoothness-weight", "0.1"]))
    assert head is not None and "warp_convention" not in head
    head = header_record(ap.parse_args(["--census-weight", "0.5", "--warp-convention", "image"]))
    assert head["warp_convention"] == "image" and head["census_weight"] == 0.5


# ---------------------------------------------------------------- the C ABI -------------
def _host(nfloats, fill):
    raw = (C.c_float * (nfloats + 8))(*([fill] * (nfloats + 8)))
    base = C.addressof(raw)
    return raw, base + (-base) % 16


@pytest.mark.parametrize("entry", ["warp_fwd", "warp_bwd", "warp_bwd_det", "photo_fwd",
                                   "photo_bwd", "census_fwd"])
@pytest.mark.parametrize("code", [2, -1])
def test_cv_entry_points_refuse_an_unknown_convention(lib, entry, code):
    """OF_EINVAL with a message naming the convention before any launch: the pointers are host
    buffers (a launch would fault), and the outputs keep their fill."""
    from optical_flow_amd._lib import OF_EINVAL
    n, h, w, c = 1, 4, 6, 8
    keep = [_host(n * h * w * c, 7.0) for _ in range(6)]
    b = [a for _, a in keep]
    P = C.c_void_p
    hs, ws = (C.c_int * 1)(h), (C.c_int * 1)(w)
    one = lambda a: (P * 1)(a)
    coef = (C.c_float * 1)(1.0)
    if entry == "warp_fwd":
        st = lib.of_warp_fwd_cv(b[0], n, h, w, c, b[1], b[2], code, None)
    elif entry == "warp_bwd":
        st = lib.of_warp_bwd_cv(b[0], b[1], n, h, w, c, b[2], b[3], b[4], None, 0, code, None)
    elif entry == "warp_bwd_det":
        st = lib.of_warp_bwd_det_cv(b[0], b[1], n, h, w, c, b[2], b[3], b[4], None, 0, code,
                                    b[5], lib.of_warp_bwd_det_workspace(n, h, w, c), None)
    elif entry == "photo_fwd":
        st = lib.of_photo_l1_fwd_multi_cv(one(b[0]), one(b[1]), n, hs, ws, 1, b[2], code, None)
    elif entry == "photo_bwd":
        st = lib.of_photo_l1_bwd_multi_cv(one(b[0]), one(b[1]), n, hs, ws, 1, coef, None,
                                          one(b[2]), (C.c_int * 1)(2), code, None)
    else:
        st = lib.of_census_fwd_multi_cv(one(b[0]), one(b[1]), n, hs, ws, 1, 1, coef, None,
                                        one(b[2]), b[3], code, None)
    assert st == OF_EINVAL, (st, lib.of_last_error())
    assert b"convention" in lib.of_last_error(), lib.of_last_error()
    for raw, _ in keep:
        assert all(v == 7.0 for v in raw)
