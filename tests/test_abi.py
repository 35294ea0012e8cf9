"""The C-ABI library (liboflow.so) loads, exports every symbol include/oflow.h declares, and
its host-only entry points behave -- no GPU compute is launched here."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from optical_flow_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def declared():
    src = open(os.path.join(ROOT, "include", "oflow.h")).read()
    return sorted(set(re.findall(r"\b(of_[a-z0-9_]+)\s*\(", src)))


def test_exports_every_declared_symbol(lib):
    from optical_flow_amd._lib import PROTOTYPES
    names = declared()
    assert len(names) >= 40
    for n in names:
        assert hasattr(lib, n), "liboflow.so does not export %s" % n
        assert n in PROTOTYPES, "ctypes binding missing for %s" % n
    assert set(PROTOTYPES) == set(names), "bindings for undeclared symbols"


def test_abi_version_and_errors(lib):
    assert lib.of_abi_version() == 1
    st = lib.of_same_pads(0, 3, 1, None, None, None)
    assert st == 1                                   # OF_EINVAL, no exception across the ABI
    assert b"same_pads" in lib.of_last_error()


def test_same_pads_tf_rule(lib):
    b, a, o = C.c_int(), C.c_int(), C.c_int()
    for n, k, s, exp in [(384, 7, 2, (2, 3, 192)), (96, 3, 2, (0, 1, 48)), (96, 1, 2, (0, 0, 48)),
                         (48, 3, 1, (1, 1, 48)), (7, 3, 2, (1, 1, 4))]:
        assert lib.of_same_pads(n, k, s, C.byref(b), C.byref(a), C.byref(o)) == 0
        assert (b.value, a.value, o.value) == exp


def test_packed_sizes_and_workspaces(lib):
    from optical_flow_amd._lib import ConvDesc
    d = ConvDesc(8, 192, 256, 115, 116, 128, 3, 3, 1, 1, 1, 192, 256)
    assert lib.of_conv_wfwd_elems(C.byref(d)) == 1056 * 128    # 9*116 -> 1044 -> 1056 rows
    assert lib.of_conv_wbwd_elems(C.byref(d)) == 9 * 128 * 116
    assert lib.of_conv2d_fwd_workspace(C.byref(d)) == 0          # big grid: no split-K
    assert lib.of_conv2d_wgrad_workspace(C.byref(d)) > 0
    small = ConvDesc(8, 24, 32, 305, 308, 128, 3, 3, 1, 1, 1, 24, 32)
    assert lib.of_conv2d_fwd_workspace(C.byref(small)) > 0       # 48 tiles: split-K
    s2 = ConvDesc(16, 96, 128, 64, 64, 128, 3, 3, 2, 0, 0, 48, 64)
    # stride-2 input grad: 4 phase groups with 4/2/2/1 taps, each padded to 16 rows
    assert lib.of_conv_wbwd_elems(C.byref(s2)) == (4 + 2 + 2 + 1) * 128 * 64
    bad = ConvDesc(1, 8, 8, 3, 3, 8, 3, 3, 1, 1, 1, 8, 8)        # cin_p not a multiple of 4
    assert lib.of_conv_wfwd_elems(C.byref(bad)) == -1


def test_pack_table_host_side(lib):
    from optical_flow_amd._lib import ConvDesc
    n = 2
    descs = (ConvDesc * n)(ConvDesc(1, 16, 16, 3, 4, 64, 7, 7, 2, 2, 2, 8, 8),
                           ConvDesc(1, 16, 16, 64, 64, 64, 3, 3, 1, 1, 1, 16, 16))
    ptrs = [(C.c_void_p * n)(16, 32) for _ in range(3)]
    buf = (C.c_char * lib.of_conv_pack_table_bytes(n))()
    assert lib.of_conv_pack_table(n, descs, *ptrs, buf) == 0
    total = C.c_int64.from_buffer(buf, 8).value
    e0 = lib.of_conv_wfwd_elems(C.byref(descs[0])) + lib.of_conv_wbwd_elems(C.byref(descs[0]))
    e1 = lib.of_conv_wfwd_elems(C.byref(descs[1])) + lib.of_conv_wbwd_elems(C.byref(descs[1]))
    assert total == e0 + e1


def _host(nfloats):
    """(keep-alive, 16-byte aligned address) of a host float buffer."""
    raw = (C.c_float * (nfloats + 8))()
    base = C.addressof(raw)
    return raw, base + (-base) % 16


# The conv entry points' stride and alignment contract (include/oflow.h): each bad argument
# is refused with OF_EINVAL and a message naming it before anything touches the device.  The
# pointers are fully sized host buffers; d: 1 x 8 x 8, 14 -> 16 input channels, 30 outputs
# (round_up(cout, 4) = 32), 3 x 3 stride 1.
_FWD_OK = dict(ldx=16, ldr=30, ldz=30, ldy=30, x_off=0, res=True, z=True)
_DG_OK = dict(lddy=32, ld_act=16, lddx=16, dy_off=0, dx_off=0)
_WG_OK = dict(ldx=16, lddy=32, x_off=0, dy_off=0)


@pytest.mark.parametrize("entry,bad,names", [
    ("fwd", dict(ldx=12), b"ldx"),                      # ldx < cin_p
    ("fwd", dict(ldx=18), b"ldx"),                      # ldx % 4 != 0
    ("fwd", dict(ldy=29), b"ldy"),                      # ldy < cout
    ("fwd", dict(ldr=29), b"ldr"),                      # ldr < cout with a residual
    ("fwd", dict(ldz=29), b"ldz"),                      # ldz < cout with z
    ("fwd", dict(x_off=4), b"x "),                      # x not 16-byte aligned
    ("dgrad", dict(lddy=28), b"lddy"),                  # lddy < round_up(cout, 4)
    ("dgrad", dict(lddy=34), b"lddy"),                  # lddy % 4 != 0
    ("dgrad", dict(lddx=15), b"lddx"),                  # lddx < cin_p
    ("dgrad", dict(ld_act=15), b"ld_act"),              # ld_act < cin_p
    ("dgrad", dict(dy_off=8), b"dy "),                  # dy not 16-byte aligned
    ("dgrad_add", dict(ld_add=15), b"ld_add"),          # ld_add < cin_p
    ("dgrad_add", dict(lddx=12), b"lddx"),
    ("wgrad", dict(ldx=12), b"ldx"),
    ("wgrad", dict(ldx=18), b"ldx"),
    ("wgrad", dict(lddy=28), b"lddy"),
    ("wgrad", dict(lddy=34), b"lddy"),
    ("wgrad", dict(x_off=4), b"x "),
    ("wgrad", dict(dy_off=12), b"dy "),
    # the Cout <= 4 layers' input gradient stores float4 rows: lddx % 4, ld_act % 4, aligned dx
    ("dgrad", dict(cout=2, lddy=4, lddx=17), b"dx"),
    ("dgrad", dict(cout=2, lddy=4, ld_act=18), b"act_src"),
    ("dgrad", dict(cout=2, lddy=4, dx_off=4), b"dx"),
], ids=lambda v: None if isinstance(v, bytes) else
    v if isinstance(v, str) else ",".join("%s=%s" % kv for kv in v.items()))
def test_conv_stride_contract(lib, entry, bad, names):
    from optical_flow_amd._lib import ConvDesc, OF_EINVAL
    cout = bad.get("cout", 30)
    d = ConvDesc(1, 8, 8, 14, 16, cout, 3, 3, 1, 1, 1, 8, 8)
    assert lib.of_conv_path(C.byref(d)) == (1 if cout <= 4 else 0)
    keep, big = _host(64 * 64 + 64)                     # 64 pixels of up to 64 floats, + offsets
    bufs = [_host(64 * 64 + 64) for _ in range(4)]
    wk, w = _host(9 * 16 * 32 * 4)
    wsk, ws = _host(1 << 20)
    if entry == "fwd":
        a = dict(_FWD_OK, **bad)
        st = lib.of_conv2d_fwd(C.byref(d), big + a["x_off"], a["ldx"], w, None, None, None, None,
                               None, 1e-3, bufs[0][1], a["ldr"], 0, 0.0, bufs[1][1], a["ldz"],
                               bufs[2][1], a["ldy"], None, 0, None)
    elif entry == "dgrad":
        a = dict(_DG_OK, **bad)
        st = lib.of_conv2d_dgrad(C.byref(d), big + a["dy_off"], a["lddy"], w, bufs[0][1],
                                 a["ld_act"], 1, 0.0, bufs[1][1] + a["dx_off"], a["lddx"], None, 0,
                                 None)
    elif entry == "dgrad_add":
        a = dict(dict(lddy=32, ld_add=16, lddx=16), **bad)
        st = lib.of_conv2d_dgrad_add(C.byref(d), big, a["lddy"], w, bufs[0][1], a["ld_add"],
                                     bufs[1][1], a["lddx"], None, 0, None)
    else:
        a = dict(_WG_OK, **bad)
        st = lib.of_conv2d_wgrad(C.byref(d), big + a["x_off"], a["ldx"], bufs[0][1] + a["dy_off"],
                                 a["lddy"], bufs[1][1], bufs[2][1], 0, ws, 1 << 22, None)
    assert st == OF_EINVAL, (st, lib.of_last_error())
    assert names in lib.of_last_error(), lib.of_last_error()


def test_photo_partials(lib):
    assert lib.of_photo_l1_partials(8, 192, 256) == (8 * 192 * 256 + 1023) // 1024


def test_product_path_refuses_cpu_tensors(lib):
    import torch
    from optical_flow_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.warp(torch.zeros(1, 4, 4, 8), torch.zeros(1, 4, 4, 2))
