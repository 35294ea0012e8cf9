"""Host side of the second-order flow smoothness term: the partials count, the argument checks
of the two C entry points (OF_EINVAL before any launch -- no GPU work here), the order argument
of LossLayer and of the ops entries, and the train command's flag and log header."""
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


def test_partials_count(lib):
    """One partial per 8 x 32 tile per image; 0 for a non-positive size."""
    for bad in [(0, 8, 32), (2, 0, 32), (2, 8, 0), (-1, 8, 32), (2, -3, 32), (2, 8, -1)]:
        assert lib.of_flow_smooth2_partials(*bad) == 0
    for (n, h, w), want in [((1, 1, 1), 1), ((2, 8, 32), 2), ((2, 9, 33), 8), ((2, 17, 70), 18),
                            ((3, 40, 57), 30), ((2, 33, 65), 30), ((8, 192, 256), 1536)]:
        assert want == n * -(-h // 8) * -(-w // 32)
        assert lib.of_flow_smooth2_partials(n, h, w) == want


def _args(lib, fn, **over):
    """A call of ``fn`` ("fwd" / "bwd") whose arguments are all valid except ``over``; the
    pointers are host buffers, which no call here ever reaches a launch with."""
    L = over.get("levels", 2)
    n_arr = max(L, 1)
    buf = (C.c_float * 64)()
    base = C.addressof(buf)
    ptrs = lambda: (C.c_void_p * n_arr)(*[base] * n_arr)
    a = dict(img6s=ptrs(), flows=ptrs(), n=2, hs=(C.c_int * n_arr)(*[3] * n_arr),
             ws=(C.c_int * n_arr)(*[4] * n_arr), levels=L, edge_alpha=0.0, eps=1e-4,
             coefs_v=(C.c_float * n_arr)(*[1.0] * n_arr),
             coefs_h=(C.c_float * n_arr)(*[1.0] * n_arr), partials=base, dloss=None,
             dflows=ptrs(), lds=(C.c_int * n_arr)(*[2] * n_arr), accumulate=0, keep=buf)
    a.update(over)
    head = (a["img6s"], a["flows"], a["n"], a["hs"], a["ws"], a["levels"], a["edge_alpha"],
            a["eps"], a["coefs_v"], a["coefs_h"])
    if fn == "fwd":
        return lib.of_flow_smooth2_fwd_multi(*head, a["partials"], None)
    return lib.of_flow_smooth2_bwd_multi(*head, a["dloss"], a["dflows"], a["lds"],
                                         a["accumulate"], None)


_BUF = (C.c_float * 8)()
BAD = [("levels0", dict(levels=0)), ("levels9", dict(levels=9)), ("n0", dict(n=0)),
       ("h0", dict(hs=(C.c_int * 2)(3, 0))), ("w0", dict(ws=(C.c_int * 2)(0, 4))),
       ("eps0", dict(eps=0.0)), ("eps_negative", dict(eps=-1e-4)),
       ("null_flows", dict(flows=None)),
       ("null_flow_level", dict(flows=(C.c_void_p * 2)(C.addressof(_BUF), None))),
       ("misaligned_flow", dict(flows=(C.c_void_p * 2)(C.addressof(_BUF), C.addressof(_BUF) + 4))),
       ("null_images_with_alpha", dict(img6s=None, edge_alpha=10.0))]


@pytest.mark.parametrize("fn", ["fwd", "bwd"])
@pytest.mark.parametrize("name,over", BAD, ids=[b[0] for b in BAD])
def test_einval(lib, fn, name, over):
    assert _args(lib, fn, **over) == 1                    # OF_EINVAL, no exception, no launch
    assert ("of_flow_smooth2_%s_multi" % fn).encode() in lib.of_last_error()


def test_einval_null_partials(lib):
    assert _args(lib, "fwd", partials=None) == 1
    assert b"of_flow_smooth2_fwd_multi" in lib.of_last_error()


@pytest.mark.parametrize("over", [dict(lds=(C.c_int * 2)(4, 1)), dict(dflows=None), dict(lds=None),
                                  dict(dflows=(C.c_void_p * 2)(C.addressof(_BUF), None))],
                         ids=["row_stride_1", "null_dflows", "null_lds", "null_dflow_level"])
def test_einval_bwd_outputs(lib, over):
    assert _args(lib, "bwd", **over) == 1
    assert b"of_flow_smooth2_bwd_multi" in lib.of_last_error()


# ------------------------------------------------------------------ the order argument ----
BAD_ORDERS = [0, 3, "2"]


@pytest.mark.parametrize("order", BAD_ORDERS)
def test_loss_layer_rejects_order(order):
    from optical_flow_amd.loss import LossLayer
    with pytest.raises(ValueError):
        LossLayer(0.2, 10, smoothness_order=order)
    with pytest.raises(ValueError):       # checked even while the weight is 0
        LossLayer(smoothness_order=order)


@pytest.mark.parametrize("order", BAD_ORDERS)
def test_ops_reject_order(order):
    """The order is checked before any tensor is looked at: no GPU is needed."""
    from optical_flow_amd import ops
    with pytest.raises(ValueError):
        ops.flow_smoothness(None, [], order=order)
    with pytest.raises(ValueError):
        ops.flow_loss(None, [], 0.2, smoothness_order=order)
    with pytest.raises(ValueError):
        ops.census_flow_loss(None, [], 1.0, smoothness_order=order)


def test_loss_layer_order_default_and_last_argument():
    import inspect
    from optical_flow_amd.loss import LossLayer
    assert LossLayer().smoothness_order == 1
    assert LossLayer(0.2, 10, smoothness_order=2).smoothness_order == 2
    assert list(inspect.signature(LossLayer.__init__).parameters)[-1] == "smoothness_order"


def test_loss_layer_passes_the_order_on_all_three_paths(monkeypatch):
    """Order 2 reaches ops.flow_loss and both ops.census_flow_loss call sites (with and without
    occlusion masks) as smoothness_order=2; order 1 adds nothing to the calls, and with
    smoothness_weight 0 the photometric fast path is taken whatever the order."""
    import torch
    from optical_flow_amd import ops
    from optical_flow_amd.loss import LossLayer
    calls = []
    for name in ("photometric_loss", "flow_loss", "census_flow_loss"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **kw: calls.append((_n, kw)) or _n)
    monkeypatch.setattr(ops, "occlusion_masks", lambda *a, **kw: ["m0", "m1"])
    batch = torch.zeros(2, 16, 16, 6)
    flows = [torch.zeros(2, 8, 8, 2), torch.zeros(2, 4, 4, 2)]
    for order, extra in ((2, {"smoothness_order": 2}), (1, {})):
        del calls[:]
        LossLayer(0.2, 10, smoothness_order=order)(batch, flows)
        LossLayer(0.2, 10, census_weight=0.5, smoothness_order=order)(batch, flows)
        LossLayer(0.2, 10, census_weight=0.5, warp_convention="image", occlusion="border",
                  smoothness_order=order)(batch, flows)
        LossLayer(smoothness_order=order)(batch, flows)
        assert calls == [("flow_loss", extra), ("census_flow_loss", extra),
                         ("census_flow_loss", dict(weights=["m0", "m1"], **extra)),
                         ("photometric_loss", {})]


def test_ops_order_arguments_are_last():
    import inspect
    from optical_flow_amd import ops
    for fn, name in [(ops.flow_smoothness, "order"), (ops.flow_loss, "smoothness_order"),
                     (ops.census_flow_loss, "smoothness_order")]:
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == name and p[name].default == 1


def test_smooth_coefs_orders():
    from optical_flow_amd import ops
    hs, ws = [5, 2, 1], [4, 3, 7]
    assert ops._smooth_coefs(2, hs, ws, 3.0) == ops._smooth_coefs(2, hs, ws, 3.0, 1)
    cv, ch = ops._smooth_coefs(2, hs, ws, 3.0, 2)
    assert cv == [3.0 / (3 * 2 * 3 * 4 * 2), 0.0, 0.0]
    assert ch == [3.0 / (3 * 2 * 5 * 2 * 2), 3.0 / (3 * 2 * 2 * 1 * 2), 3.0 / (3 * 2 * 1 * 5 * 2)]


# --------------------------------------------------------------------- the train command ----
def test_train_help_lists_the_flag():
    r = subprocess.run([sys.executable, "-m", "optical_flow_amd.train", "--help"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--smoothness-order" in r.stdout


def test_header_record_carries_order_2_only():
    from optical_flow_amd.train import build_parser, header_record
    ap = build_parser()
    base = ["--smoothness-weight", "0.2", "--edge-alpha", "10"]
    plain = header_record(ap.parse_args(base))
    assert ap.parse_args(base).smoothness_order == 1
    assert header_record(ap.parse_args(base + ["--smoothness-order", "1"])) == plain
    assert "smoothness_order" not in plain
    two = header_record(ap.parse_args(base + ["--smoothness-order", "2"]))
    assert two.pop("smoothness_order") == 2 and two == plain
    # a default run has no header; order 2 alone is a non-default option
    assert header_record(ap.parse_args([])) is None
    assert header_record(ap.parse_args(["--smoothness-order", "1"])) is None
    assert header_record(ap.parse_args(["--smoothness-order", "2"]))["smoothness_order"] == 2
    with pytest.raises(SystemExit):
        ap.parse_args(["--smoothness-order", "3"])
