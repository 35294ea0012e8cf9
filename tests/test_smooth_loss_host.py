"""Host side of the flow smoothness term: the partials count, the argument checks of the two
C entry points (OF_EINVAL before any launch -- no GPU work here), LossLayer's argument checks
and the train command's flags."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from optical_flow_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def test_partials_positive_and_monotone(lib):
    sizes = [(1, 1, 1), (2, 1, 5), (2, 5, 7), (2, 32, 32), (2, 33, 65), (8, 96, 128),
             (8, 192, 256), (8, 384, 512)]
    sizes.sort(key=lambda s: s[0] * s[1] * s[2])
    counts = [lib.of_flow_smooth_partials(*s) for s in sizes]
    assert all(c >= 1 for c in counts)
    assert counts == sorted(counts) and counts[-1] > counts[0]


def _args(lib, fn, **over):
    """A call of ``fn`` ("fwd" / "bwd") whose arguments are all valid except ``over``; the
    pointers are host buffers, which no valid-argument call here ever reaches a launch with."""
    L = over.get("levels", 2)
    n_arr = max(L, 1)
    buf = (C.c_float * 64)()
    base = C.addressof(buf)
    a = dict(img6s=(C.c_void_p * n_arr)(*[base] * n_arr), flows=(C.c_void_p * n_arr)(*[base] * n_arr),
             n=2, hs=(C.c_int * n_arr)(*[3] * n_arr), ws=(C.c_int * n_arr)(*[4] * n_arr), levels=L,
             edge_alpha=0.0, eps=1e-4, coefs_v=(C.c_float * n_arr)(*[1.0] * n_arr),
             coefs_h=(C.c_float * n_arr)(*[1.0] * n_arr), partials=base, dloss=None,
             dflows=(C.c_void_p * n_arr)(*[base] * n_arr), lds=(C.c_int * n_arr)(*[2] * n_arr),
             accumulate=0, keep=buf)
    a.update(over)
    head = (a["img6s"], a["flows"], a["n"], a["hs"], a["ws"], a["levels"], a["edge_alpha"],
            a["eps"], a["coefs_v"], a["coefs_h"])
    if fn == "fwd":
        return lib.of_flow_smooth_fwd_multi(*head, a["partials"], None)
    return lib.of_flow_smooth_bwd_multi(*head, a["dloss"], a["dflows"], a["lds"], a["accumulate"],
                                        None)


BAD = [("levels0", dict(levels=0)), ("levels9", dict(levels=9)), ("n0", dict(n=0)),
       ("h0", dict(hs=(C.c_int * 2)(3, 0))), ("w0", dict(ws=(C.c_int * 2)(0, 4))),
       ("eps0", dict(eps=0.0)), ("eps_negative", dict(eps=-1e-4)),
       ("null_images_with_alpha", dict(img6s=None, edge_alpha=10.0))]


@pytest.mark.parametrize("fn", ["fwd", "bwd"])
@pytest.mark.parametrize("name,over", BAD, ids=[b[0] for b in BAD])
def test_einval(lib, fn, name, over):
    assert _args(lib, fn, **over) == 1                    # OF_EINVAL, no exception, no launch
    assert ("of_flow_smooth_%s_multi" % fn).encode() in lib.of_last_error()


def test_einval_row_stride(lib):
    assert _args(lib, "bwd", lds=(C.c_int * 2)(4, 1)) == 1
    assert b"of_flow_smooth_bwd_multi" in lib.of_last_error()


@pytest.mark.parametrize("kw", [dict(smoothness_weight=-0.1), dict(edge_alpha=-1.0),
                                dict(smoothness_eps=0.0), dict(smoothness_eps=-1e-4)])
def test_loss_layer_rejects(kw):
    from optical_flow_amd.loss import LossLayer
    with pytest.raises(ValueError):
        LossLayer(**kw)


def test_loss_layer_defaults():
    from optical_flow_amd.loss import LossLayer
    d = LossLayer()
    assert (d.smoothness_weight, d.edge_alpha, d.smoothness_eps) == (0.0, 0.0, 1e-4)
    s = LossLayer(0.2, 10)
    assert (s.smoothness_weight, s.edge_alpha) == (0.2, 10.0)


def test_train_help_lists_the_flags():
    r = subprocess.run([sys.executable, "-m", "optical_flow_amd.train", "--help"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--smoothness-weight" in r.stdout and "--edge-alpha" in r.stdout
