"""The conv host planner, pinned without a GPU: every workspace / partial-sum size query of the
conv ABI, for every conv layer of the model and the small layers of test_gpu_conv_strides, under
default tuning and under each planner key taken alone, against numbers the library itself
returned (tests/golden/conv_plan_bytes.json; re-record with `python tests/test_conv_plan_host.py
--record` only when a plan is meant to change).  device_cus() is 256 without a device, so the
numbers are those of an MI355X.  of_set_tuning's accepted ranges are pinned too.  Nothing is
launched."""
import ctypes as C
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_plan_bytes.json")

# of_set_tuning: key -> (lowest, highest accepted value)
RANGES = {1: (1, 16), 2: (2, 64), 3: (0, 1), 4: (0, 2), 5: (1, 2), 6: (0, 1), 7: (0, 1), 8: (0, 2),
          9: (0, 7), 10: (1, 16), 11: (0, 1), 12: (0, 3), 13: (0, 1), 14: (0, 1), 15: (0, 1),
          16: (0, 7), 17: (0, 1), 18: (0, 1), 19: (0, 1), 20: (0, 1), 21: (0, 3), 22: (0, 1),
          23: (0, 3), 24: (0, 2), 25: (0, 1000), 26: (0, 1000), 27: (0, 100000), 28: (0, 64),
          29: (0, 4), 30: (0, 2), 31: (-1, 8), 32: (0, 1), 33: (1, 256), 34: (0, 2), 35: (0, 1),
          36: (0, 3), 37: (0, 16), 38: (0, 131072), 39: (0, 1), 40: (0, 1)}
# the keys the planner reads, with their defaults
DEFAULTS = {1: 4, 2: 12, 4: 1, 6: 1, 10: 4, 11: 1, 12: 0, 13: 0, 14: 1, 15: 1, 16: 6, 25: 5,
            26: 5, 27: 1200, 33: 2, 36: 0}
SETTINGS = [(1, 8), (2, 4), (4, 0), (4, 2), (6, 0), (10, 8), (11, 0), (12, 1), (12, 2), (13, 1),
            (14, 0), (15, 0), (16, 0), (16, 7), (25, 0), (26, 0), (27, 0), (33, 1), (33, 8),
            (36, 1), (36, 2)]
QUERIES = ["fwd", "dgrad", "fwd_bf16", "dgrad_bf16", "fwd_x3", "dgrad_x3", "wgrad", "wgrad_bf16",
           "wgrad_x3", "wgrad_bn0", "wgrad_bn1", "wgrad_bn2", "stem_fused1", "stem_fused2", "bnp"]


@pytest.fixture(scope="module")
def lib():
    from optical_flow_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def _shapes():
    """(n, h, w, cin, cout, k, stride) of every conv of the model at 384 x 512, B = 8 and at
    768 x 1024, B = 2 (walked as bench.py gflop_per_pair walks them; the encoder runs both
    images as one batch of 2 B), then the layers of test_gpu_conv_strides."""
    from optical_flow_amd.params import HEAD_WIDTHS, encoder_blocks, head_cin
    out = []
    for H, W, B in ((384, 512, 8), (768, 1024, 2)):
        out.append((2 * B, H, W, 3, 64, 7, 2))                       # the stem
        hh, ww = H // 4, W // 4                                      # after the stem and the pool
        for _, cin, cout, stride, proj in encoder_blocks(4):
            out.append((2 * B, hh, ww, cin, cout, 3, stride))        # conv_a
            ho, wo = hh // stride, ww // stride
            out.append((2 * B, ho, wo, cout, cout, 3, 1))            # conv_b
            if proj:
                out.append((2 * B, hh, ww, cin, cout, 1, stride))
            hh, ww = ho, wo
        for level in range(4):
            s = 16 >> level
            cin = head_cin(level, 3, 4)
            for cout in HEAD_WIDTHS:
                out.append((B, H // s, W // s, cin, cout, 3, 1))
                cin = cout
    from test_gpu_conv_strides import CASES
    out += [c[0] for c in CASES]
    return list(dict.fromkeys(out))


def _desc(lib, shape):
    from optical_flow_amd._lib import ConvDesc
    n, h, w, cin, cout, k, s = shape
    pt, pl, ho, wo, _ = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert lib.of_same_pads(h, k, s, C.byref(pt), C.byref(_), C.byref(ho)) == 0
    assert lib.of_same_pads(w, k, s, C.byref(pl), C.byref(_), C.byref(wo)) == 0
    return ConvDesc(n, h, w, cin, (cin + 3) // 4 * 4, cout, k, k, s, pt.value, pl.value, ho.value,
                    wo.value)


def _row(lib, d):
    p = C.byref(d)
    return [lib.of_conv2d_fwd_workspace(p), lib.of_conv2d_dgrad_workspace(p),
            lib.of_conv2d_fwd_bf16_workspace(p), lib.of_conv2d_dgrad_bf16_workspace(p),
            lib.of_conv2d_fwd_x3_workspace(p), lib.of_conv2d_dgrad_x3_workspace(p),
            lib.of_conv2d_wgrad_workspace(p), lib.of_conv2d_wgrad_bf16_workspace(p),
            lib.of_conv2d_wgrad_x3_workspace(p), lib.of_conv2d_wgrad_bn_workspace(p, 0),
            lib.of_conv2d_wgrad_bn_workspace(p, 1), lib.of_conv2d_wgrad_bn_workspace(p, 2),
            lib.of_stem_bwd_fused_workspace(p, 1), lib.of_stem_bwd_fused_workspace(p, 2),
            lib.of_conv2d_dgrad_bnp_bytes(p)]


def _reset(lib):
    for k, v in DEFAULTS.items():
        assert lib.of_set_tuning(k, v) == 0


def _measure(lib):
    """{"default": {shape: row}, "key=value": {shape: row, only where it differs from default}}"""
    shapes = _shapes()
    descs = [_desc(lib, s) for s in shapes]
    name = lambda s: "x".join(map(str, s))
    got = {}
    try:
        _reset(lib)
        base = {name(s): _row(lib, d) for s, d in zip(shapes, descs)}
        got["default"] = base
        for k, v in SETTINGS:
            _reset(lib)
            assert lib.of_set_tuning(k, v) == 0
            rows = {name(s): _row(lib, d) for s, d in zip(shapes, descs)}
            got["%d=%d" % (k, v)] = {s: r for s, r in rows.items() if r != base[s]}
    finally:
        _reset(lib)
    return got


def test_plan_bytes(lib):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert want["queries"] == QUERIES
    got = _measure(lib)
    assert set(got) == set(want["bytes"])
    for setting in got:
        assert set(got[setting]) == set(want["bytes"][setting]), setting
        for shape, row in got[setting].items():
            assert row == want["bytes"][setting][shape], (setting, shape, dict(zip(QUERIES, row)))
    assert len(got["default"]) >= 60 and any(got[s] for s in got if s != "default")
    assert _measure(lib)["default"] == got["default"], "a setting was left behind"


def test_tuning_ranges(lib):
    """Every key refuses the first value below and above its range, and keys 0 and 41 are
    unknown (a refused call changes nothing)."""
    assert sorted(RANGES) == list(range(1, 41))
    for key, (lo, hi) in RANGES.items():
        assert lib.of_set_tuning(key, lo - 1) == 1, (key, lo - 1)
        assert lib.of_set_tuning(key, hi + 1) == 1, (key, hi + 1)
        assert b"of_set_tuning" in lib.of_last_error()
    for key in (0, 41, -1):
        assert lib.of_set_tuning(key, 1) == 1, key


if __name__ == "__main__" and "--record" in sys.argv:
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from optical_flow_amd import _lib
    with open(GOLDEN, "w") as f:
        json.dump({"queries": QUERIES, "bytes": _measure(_lib.load())}, f, separators=(",", ":"))
        f.write("\n")
    print("recorded", GOLDEN)
