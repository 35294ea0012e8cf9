"""Host side of the census data term: the partials count and workspace size, the argument
checks of the two C entry points (OF_EINVAL before any launch -- no GPU work here),
LossLayer's argument checks, the train command's flags, and the float64 reference's own
properties (tests/census_ref.py) on the CPU."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import census_ref
from helpers import rng_tensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from optical_flow_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def test_partials_positive_and_monotone(lib):
    sizes = [(1, 1, 1), (2, 1, 9), (2, 5, 3), (2, 13, 21), (2, 33, 65), (8, 96, 128),
             (8, 192, 256), (8, 384, 512)]
    sizes.sort(key=lambda s: s[0] * s[1] * s[2])
    counts = [lib.of_census_partials(*s) for s in sizes]
    assert all(c >= 1 for c in counts)
    assert counts == sorted(counts) and counts[-1] > counts[0]


def test_workspace_size(lib):
    """The forward recomputes its halo: no workspace at any size (DESIGN.md "Census term"), so
    the NULL-workspace refusal of the ABI has no case to show in this build."""
    for s in [(1, 1, 1), (2, 33, 65), (8, 192, 256)]:
        assert lib.of_census_workspace_floats(*s) == 0


def _args(lib, fn, **over):
    """A call of ``fn`` ("fwd" / "bwd") whose arguments are all valid except ``over``; the
    pointers are host buffers, which no call here ever reaches a launch with."""
    L = over.get("levels", 2)
    n_arr = max(L, 1)
    buf = (C.c_float * 64)()
    base = C.addressof(buf)
    base += (-base) % 8
    ptrs = lambda: (C.c_void_p * n_arr)(*[base] * n_arr)
    a = dict(img6s=ptrs(), flows=ptrs(), n=2, hs=(C.c_int * n_arr)(*[3] * n_arr),
             ws=(C.c_int * n_arr)(*[4] * n_arr), levels=L, radius=3,
             coefs=(C.c_float * n_arr)(*[1.0] * n_arr), workspaces=None, dcdfs=ptrs(),
             partials=base, dloss=None, dflows=ptrs(), lds=(C.c_int * n_arr)(*[2] * n_arr),
             accumulate=0, keep=buf)
    a.update(over)
    if fn == "fwd":
        return lib.of_census_fwd_multi(a["img6s"], a["flows"], a["n"], a["hs"], a["ws"],
                                       a["levels"], a["radius"], a["coefs"], a["workspaces"],
                                       a["dcdfs"], a["partials"], None)
    return lib.of_census_bwd_multi(a["dcdfs"], a["n"], a["hs"], a["ws"], a["levels"], a["coefs"],
                                   a["dloss"], a["dflows"], a["lds"], a["accumulate"], None)


BAD = [("levels0", dict(levels=0)), ("levels9", dict(levels=9)), ("n0", dict(n=0)),
       ("h0", dict(hs=(C.c_int * 2)(3, 0))), ("w0", dict(ws=(C.c_int * 2)(0, 4)))]


@pytest.mark.parametrize("fn", ["fwd", "bwd"])
@pytest.mark.parametrize("name,over", BAD, ids=[b[0] for b in BAD])
def test_einval(lib, fn, name, over):
    assert _args(lib, fn, **over) == 1                    # OF_EINVAL, no exception, no launch
    assert ("of_census_%s_multi" % fn).encode() in lib.of_last_error()


@pytest.mark.parametrize("radius", [0, 4, -1])
def test_einval_radius(lib, radius):
    assert _args(lib, "fwd", radius=radius) == 1
    assert b"of_census_fwd_multi" in lib.of_last_error() and b"radius" in lib.of_last_error()


def test_einval_null_partials(lib):
    assert _args(lib, "fwd", partials=None) == 1
    assert b"of_census_fwd_multi" in lib.of_last_error() and b"partials" in lib.of_last_error()


def test_einval_row_stride(lib):
    assert _args(lib, "bwd", lds=(C.c_int * 2)(4, 1)) == 1
    assert b"of_census_bwd_multi" in lib.of_last_error() and b"lds" in lib.of_last_error()


@pytest.mark.parametrize("kw", [dict(census_weight=-0.1), dict(photometric_weight=-1.0),
                                dict(census_weight=1.0, census_radius=0),
                                dict(census_weight=1.0, census_radius=4),
                                dict(census_weight=1.0, census_radius=2.5),
                                dict(photometric_weight=0.0),
                                dict(census_weight=0.0, photometric_weight=0.0)])
def test_loss_layer_rejects(kw):
    from optical_flow_amd.loss import LossLayer
    with pytest.raises(ValueError):
        LossLayer(**kw)


def test_loss_layer_defaults():
    from optical_flow_amd.loss import LossLayer
    d = LossLayer()
    assert (d.smoothness_weight, d.edge_alpha, d.smoothness_eps) == (0.0, 0.0, 1e-4)
    assert (d.census_weight, d.census_radius, d.photometric_weight) == (0.0, 3, 1.0)
    s = LossLayer(0.2, 10, 1e-3, 0.5, 2, 0.25)          # the positional order
    assert (s.smoothness_weight, s.edge_alpha, s.smoothness_eps) == (0.2, 10.0, 1e-3)
    assert (s.census_weight, s.census_radius, s.photometric_weight) == (0.5, 2, 0.25)
    assert LossLayer(census_weight=1.0, photometric_weight=0.0).photometric_weight == 0.0


def test_train_help_lists_the_flags():
    r = subprocess.run([sys.executable, "-m", "optical_flow_amd.train", "--help"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ("--census-weight", "--census-radius", "--photometric-weight"):
        assert flag in r.stdout


# --------------------------------------------------- the reference's own properties ----
@pytest.mark.parametrize("shape,r", [((2, 9, 11), 3), ((1, 5, 3), 3), ((2, 6, 7), 1),
                                     ((2, 1, 9), 2)])
def test_closed_form_gradient_is_autograd(shape, r):
    """dC/du by the closed form the kernel uses against autograd of the definition."""
    g1 = rng_tensor(shape, 11, scale=20.0).double()
    u = rng_tensor(shape, 12, scale=20.0).double().requires_grad_(True)
    c = census_ref.level_sum(g1, u, r)
    c.backward()
    c2, grad = census_ref.level_closed_form(g1, u.detach(), r)
    assert abs(c2.item() - c.item()) <= 1e-12 * abs(c.item())
    assert (grad - u.grad).norm().item() <= 1e-12 * u.grad.norm().item()


def test_single_pixel_level_contributes_nothing():
    img = rng_tensor((2, 1, 1, 6), 3, lo=-0.5, hi=0.6).double()
    f = rng_tensor((2, 1, 1, 2), 4, scale=3.0).double().requires_grad_(True)
    g1, u = census_ref.gray_pair(img, f)
    c = census_ref.level_sum(g1, u, 3)
    assert c.item() == 0.0
    # a level with no pairs has no graph to the flow at all
    assert not c.requires_grad


def _transposed_pair(n, s, offset):
    i1 = rng_tensor((n, s, s, 3), 21, lo=-0.5, hi=0.6).double()
    return torch.cat([i1, i1.transpose(1, 2) + offset], -1)


def test_identity_case():
    """Zero flow samples image 2 transposed (P1): with image 2 = image 1 transposed the warped
    image is image 1, value and gradient exactly 0."""
    img = _transposed_pair(2, 12, 0.0)
    f = torch.zeros(2, 12, 12, 2, dtype=torch.float64, requires_grad=True)
    g1, u = census_ref.gray_pair(img, f)
    assert torch.equal(g1, u)
    c = census_ref.level_sum(g1, u, 3)
    c.backward()
    assert c.item() == 0.0 and (f.grad == 0).all()


def test_offset_case():
    """A brightness offset on image 2 moves the photometric L1 by the offset and the census
    term not at all (up to rounding)."""
    from oracle import ref_flow as R
    img = _transposed_pair(2, 12, 0.125)
    f = torch.zeros(2, 12, 12, 2, dtype=torch.float64)
    g1, u = census_ref.gray_pair(img, f)
    assert census_ref.level_sum(g1, u, 3).item() / (2 * 12 * 12) < 1e-9
    l1 = (img[..., :3] - R.warp_features(f, img[..., 3:])).abs().mean().item()
    assert abs(l1 - 0.125) < 1e-12
