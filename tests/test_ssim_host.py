"""Host side of the SSIM data term: the closed-form gradient against autograd, the bound on S
and the float32 conditioning of every input the GPU tests use (tests/ssim_cases.py),
LossLayer's argument checks, the train command's flag and header record, the normaliser of a
level without windows, and the argument checks of the C entry (OF_EINVAL before any launch --
no GPU work here)."""
import ctypes as C
import os

import pytest
import torch

import occlusion_ref
import ssim_cases
import ssim_ref
from helpers import REL_TOL, f64, rel_l2, rng_tensor
from oracle import ref_flow as R


# ------------------------------------------------------- the reference's own properties ----
@pytest.mark.parametrize("shape", [(2, 3, 3), (1, 5, 3), (2, 3, 9), (2, 9, 11), (1, 13, 21)])
def test_closed_form_gradient_is_autograd(shape):
    """d SSIM_l / d y by the closed form the kernel uses against float64 autograd of the
    definition, with random centre weights."""
    x = rng_tensor(shape + (3,), 11, lo=0.0, hi=1.0).double()
    y = rng_tensor(shape + (3,), 12, lo=0.0, hi=1.0).double().requires_grad_(True)
    m = rng_tensor(shape, 13, lo=0.0, hi=2.0).double()
    s = ssim_ref.level_sum(x, y, m)
    s.backward()
    s2, grad = ssim_ref.level_closed_form(x, y.detach(), m)
    assert abs(s2.item() - s.item()) <= 1e-10 * abs(s.item())
    assert (grad - y.grad).norm().item() <= 1e-10 * y.grad.norm().item()


def _all_level_inputs():
    """(name, convention, image level, flow level) of every ABI-level GPU input."""
    for kind, (imgs, flows) in (("textured", ssim_cases.textured()),
                                ("low", ssim_cases.low_texture())):
        for cv in ssim_cases.CONVENTIONS:
            for im, f in zip(imgs, flows):
                yield "%s %s %s" % (kind, cv, tuple(f.shape[1:3])), cv, im, f
    for levels in (4, 5):
        batch, flows = ssim_cases.pyramid_case(levels)
        for cv in ssim_cases.CONVENTIONS:
            for f in flows:
                im = R.resize_bilinear(batch, f.shape[1], f.shape[2])
                yield "pyramid%d %s %s" % (levels, cv, tuple(f.shape[1:3])), cv, im, f
    for mode in ("border", "fb"):              # the occlusion tests' conditioned flows
        batch, flows = occlusion_ref.layer_case(mode)
        for f in flows:
            im = R.resize_bilinear(batch, f.shape[1], f.shape[2])
            yield "occlusion %s %s" % (mode, tuple(f.shape[1:3])), "image", im, f


def test_s_is_bounded_on_the_gpu_inputs():
    """S in [-1,1] (|2 mx my| <= mx^2 + my^2, |2 sxy| <= sx + sy): d needs no clamp."""
    lo, hi = 1.0, -1.0
    for name, cv, im, f in _all_level_inputs():
        if f.shape[1] < 3 or f.shape[2] < 3:
            continue
        with ssim_cases.convention(cv):
            s = ssim_ref.structural_similarity(*ssim_ref.intensities(f64(im), f64(f)))
        lo, hi = min(lo, s.min().item()), max(hi, s.max().item())
        assert -1.0 <= s.min().item() and s.max().item() <= 1.0, name
    print("S range over the GPU inputs: [%.4f, %.4f]" % (lo, hi))


def test_float32_reference_is_well_conditioned_on_the_gpu_inputs():
    """A float32 torch evaluation of the reference is within REL_TOL / 10 of float64 on every
    GPU input, value and d(flow): REL_TOL then has a factor 10 left for the kernel."""
    worst = (0.0, 0.0)
    for name, cv, im, f in _all_level_inputs():
        v64, g64 = ssim_cases.level_value_grad(f64(im), f64(f), cv)
        v32, g32 = ssim_cases.level_value_grad(im, f, cv)
        if v64 == 0.0:
            assert v32 == 0.0 and not g32.any(), name
            continue
        ev, eg = abs(v32 - v64) / abs(v64), rel_l2(g32, g64)
        worst = (max(worst[0], ev), max(worst[1], eg))
        assert ev < REL_TOL / 10 and eg < REL_TOL / 10, (name, ev, eg)
    print("float32 against float64, worst value %.2e, worst d(flow) %.2e" % worst)


def test_windowless_level_has_coefficient_zero():
    from optical_flow_amd import ops
    co = ops._ssim_coefs(2, [32, 3, 2, 5], [64, 3, 4, 2], 0.85)
    assert co[2] == 0.0 and co[3] == 0.0
    assert co[0] == pytest.approx(0.85 / (4 * 2 * 30 * 62 * 3))
    assert co[1] == pytest.approx(0.85 / (4 * 2 * 1 * 1 * 3))
    assert ssim_ref.level_coef(2, 2, 4) == 0.0 and ssim_ref.level_coef(2, 1, 1) == 0.0
    x = rng_tensor((2, 2, 4, 3), 1, lo=0.0, hi=1.0).double().requires_grad_(True)
    s = ssim_ref.level_sum(x, x + 0.1)
    assert s.item() == 0.0 and not s.requires_grad


def test_known_answer_constant_images():
    """x = a, y = b everywhere: sigma = 0, S = (2ab + C1)/(a^2 + b^2 + C1), the loss
    (a-b)^2 / (2 (a^2 + b^2 + C1)) = 0.027023 for 0.5 / 0.7."""
    x = torch.full((1, 5, 6, 3), 0.5, dtype=torch.float64)
    y = torch.full((1, 5, 6, 3), 0.7, dtype=torch.float64)
    got = ssim_ref.level_sum(x, y).item() * ssim_ref.level_coef(1, 5, 6)
    want = (0.5 - 0.7) ** 2 / (2 * (0.25 + 0.49 + ssim_ref.C1))
    assert abs(got - want) < 1e-14 and abs(want - 0.027023) < 5e-7


# ------------------------------------------------------------------------ LossLayer ----
@pytest.mark.parametrize("kw", [dict(ssim_weight=-0.1), dict(ssim_weight=float("nan")),
                                dict(photometric_weight=0.0),
                                dict(photometric_weight=0.0, census_weight=0.0,
                                     ssim_weight=0.0)])
def test_loss_layer_rejects(kw):
    from optical_flow_amd.loss import LossLayer
    with pytest.raises(ValueError):
        LossLayer(**kw)


def test_loss_layer_accepts_ssim_as_the_only_data_term():
    from optical_flow_amd.loss import LossLayer
    assert LossLayer().ssim_weight == 0.0
    d = LossLayer(photometric_weight=0.0, ssim_weight=1.0)
    assert (d.ssim_weight, d.photometric_weight, d.census_weight) == (1.0, 0.0, 0.0)
    d = LossLayer(photometric_weight=0.15, ssim_weight=0.85, warp_convention="image",
                  occlusion="border")
    assert (d.ssim_weight, d.photometric_weight, d.occlusion) == (0.85, 0.15, "border")


def test_census_flow_loss_needs_one_of_three_data_terms():
    from optical_flow_amd import ops
    with pytest.raises(AssertionError, match="data term"):
        ops.census_flow_loss(None, [], 0.0, photometric_weight=0.0, ssim_weight=0.0)


# ------------------------------------------------------------------ train command ----
def test_parser_and_header_record():
    from optical_flow_amd.train import build_parser, header_record
    ap = build_parser()
    assert ap.parse_args([]).ssim_weight == 0.0
    assert header_record(ap.parse_args([])) is None
    args = ap.parse_args(["--photometric-weight", "0.15", "--ssim-weight", "0.85"])
    head = header_record(args)
    assert head["ssim_weight"] == 0.85 and head["photometric_weight"] == 0.15
    assert head["header"] is True
    # the key appears only when the term is on: other logs stay what they were
    assert "ssim_weight" not in header_record(ap.parse_args(["--census-weight", "1"]))
    assert header_record(ap.parse_args(["--ssim-weight", "0.5"])) == {
        "header": True, "smoothness_weight": 0.0, "edge_alpha": 0.0, "ssim_weight": 0.5}


# ------------------------------------------------------------ the C entry's checks ----
@pytest.fixture(scope="module")
def lib():
    from optical_flow_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def test_partials_count(lib):
    assert lib.of_ssim_partials(3, 1, 1) == 3 and lib.of_ssim_partials(3, 40, 57) == 3 * 5 * 2
    assert lib.of_ssim_partials(2, 8, 32) == 2 and lib.of_ssim_partials(2, 9, 33) == 8
    assert lib.of_ssim_partials(0, 8, 32) == 0


def _fwd(lib, **over):
    """of_ssim_fwd_multi with every argument valid except ``over``; the pointers are host
    buffers, which no call here ever reaches a launch with."""
    L = over.get("levels", 2)
    k = max(L, 1)
    buf = (C.c_float * 64)()
    base = C.addressof(buf)
    base += (-base) % 8
    ptrs = lambda: (C.c_void_p * k)(*[base] * k)
    a = dict(img6s=ptrs(), flows=ptrs(), weights=None, n=2, hs=(C.c_int * k)(*[3] * k),
             ws=(C.c_int * k)(*[4] * k), levels=L, coefs=(C.c_float * k)(*[1.0] * k),
             dsdfs=ptrs(), partials=base, convention=0)
    a.update(over)
    return lib.of_ssim_fwd_multi(a["img6s"], a["flows"], a["weights"], a["n"], a["hs"], a["ws"],
                                 a["levels"], a["coefs"], a["dsdfs"], a["partials"],
                                 a["convention"], None)


def _null_entry():
    p = (C.c_void_p * 2)()
    buf = (C.c_float * 8)()
    p[0] = C.addressof(buf)
    p._keep = buf
    return p                                   # entry 1 is NULL


BAD = [("levels0", dict(levels=0)), ("levels9", dict(levels=9)), ("n0", dict(n=0)),
       ("h0", dict(hs=(C.c_int * 2)(3, 0))), ("w0", dict(ws=(C.c_int * 2)(0, 4))),
       ("convention2", dict(convention=2)), ("convention-1", dict(convention=-1)),
       ("img6s", dict(img6s=None)), ("flows", dict(flows=None)), ("partials", dict(partials=None)),
       ("img6s[1]", dict(img6s=_null_entry())), ("flows[1]", dict(flows=_null_entry()))]


@pytest.mark.parametrize("name,over", BAD, ids=[b[0] for b in BAD])
def test_einval(lib, name, over):
    assert _fwd(lib, **over) == 1                      # OF_EINVAL, no exception, no launch
    assert b"of_ssim_fwd_multi" in lib.of_last_error()
