"""The 3-tap weight gradient's two x-halo stagings give bitwise the same sums.

conv_wgrad_tile_x3 stages the x halo as one pixel-major image read with transposing LDS reads,
double-buffered (of_set_tuning key 40 = 1, the default); conv_wgrad_tile_x3_c3 keeps the three
pixel-shifted copies (key 40 = 0).  Both feed the same MFMA sequence with the same operands, so
dw and db must be torch.equal, not merely close.  Each case runs the weight gradient through
the C ABI (of_conv2d_wgrad_x3) with key 40 = 0 and = 1 into NaN-filled dw, db and workspace,
requires finite and equal results, reads the timing kind back to make sure the 3-tap kernel of
that channel-block shape ran, and checks the centre tap against an fp64 einsum.

Shapes: the smallest at which the image can go wrong -- one whole tile; a shape smaller than a
tile (zero halo on all four sides); partial tiles and a ragged second channel block, with row
strides larger than the channel counts and NaN in the gaps; slices of >= 4 tiles (the double
buffer's prologue, steady state and last tile); every instantiation (CIB 32 / 64, XH 8 / 4,
COB 128 / 96 / 64 / 32).
"""
import ctypes as C
import zlib

import pytest
import torch

from helpers import REL_TOL, rel_inf, rng_tensor

pytestmark = pytest.mark.gpu

STAGE_KEY = 40
# of_set_tuning defaults of the keys the cases change (conv_f32.hip)
DEFAULTS = {4: 1, 11: 1, 33: 2, STAGE_KEY: 1}

# ((n, h, w, cin, cout), {key: value}, timing kind, (ldx - cin_p, lddy - cout_p))
CASES = [
    ((1, 8, 16, 32, 96), {}, 145, (0, 0)),          # one whole tile, <1, 3, 3, 8>
    ((1, 5, 7, 32, 96), {}, 145, (0, 0)),           # smaller than a tile: zero halo on four sides
    ((2, 9, 17, 40, 96), {}, 145, (24, 12)),        # partial tiles, ragged block; strides
    ((3, 24, 32, 64, 96), {33: 4}, 145, (0, 0)),    # slices of >= 4 tiles
    ((2, 16, 32, 64, 64), {}, 146, (0, 0)),         # <2, 2, 3, 4>: CIB 64, XH 4
    # CIB 64 with a partly empty second block, partial tiles (key 11 = 0: a Cin that is no
    # multiple of 64 otherwise takes the 9-tap 32 x 64 blocks, kind 152)
    ((2, 9, 17, 72, 64), {11: 0}, 146, (0, 0)),
    ((2, 16, 32, 64, 32), {}, 147, (0, 0)),         # <2, 1, 3, 4>
    ((1, 8, 16, 32, 128), {4: 0}, 144, (0, 0)),     # <1, 4, 3, 8>: only with key 4 = 0
]
_ID = lambda c: "x".join(map(str, c[0])) + "".join("-k%d=%d" % kv for kv in c[1].items())


def _timing_kinds(lib):
    cap = 64
    k = (C.c_int * cap)()
    cnt = lib.of_timing_read(cap, k, None, None)
    assert cnt < cap
    return [k[i] for i in range(cnt)]


@pytest.mark.parametrize("case", CASES, ids=_ID)
def test_wgrad3_stage_bitwise(case):
    from optical_flow_amd import _lib, ops
    from optical_flow_amd._lib import ACT_NONE, call
    (n, h, w, cin, cout), keys, kind, (gx, gd) = case
    lib = _lib.lib()
    assert set(keys) <= set(DEFAULTS)
    seed = zlib.crc32(repr((n, h, w, cin, cout)).encode()) % 1000 + 1500
    cin_p, cout_p = (cin + 3) // 4 * 4, (cout + 3) // 4 * 4
    ldx, lddy = cin_p + gx, cout_p + gd
    nan = float("nan")
    # rows of ldx / lddy floats: the data in the first cin / cout channels, zero padding up to
    # cin_p / cout_p, NaN in the gap that a strided parent would hold
    x = torch.full((n, h, w, ldx), nan)
    x[..., :cin_p] = 0
    x[..., :cin] = rng_tensor((n, h, w, cin), seed)
    dy = torch.full((n, h, w, lddy), nan)
    dy[..., :cout_p] = 0
    dy[..., :cout] = rng_tensor((n, h, w, cout), seed + 1)
    x, dy = x.cuda(), dy.cuda()
    wt = rng_tensor((3, 3, cin, cout), seed + 2, scale=(2.0 / (9 * cin)) ** 0.5).cuda()
    bias = rng_tensor((cout,), seed + 3, scale=0.1).cuda()
    P, st = ops._ptr, ops._stream()
    out = {}
    try:
        for k, v in keys.items():
            assert lib.of_set_tuning(k, v) == 0
        layer = ops.ConvLayer(wt, bias, stride=1, act=ACT_NONE, cin_p=cin_p, precision="fp32",
                              f32_split=True)
        d = layer.desc(n, h, w)
        went, wsb = layer.wgrad_entry(d)
        assert went == "of_conv2d_wgrad_x3"
        ws = torch.empty(wsb // 4 + 4, device="cuda")
        for stage in (0, 1):
            assert lib.of_set_tuning(STAGE_KEY, stage) == 0
            dw = torch.full((3, 3, cin, cout), nan, device="cuda")
            db = torch.full((cout,), nan, device="cuda")
            ws.fill_(nan)
            lib.of_timing_read(0, None, None, None)            # drop earlier records
            lib.of_timing_enable(1)
            try:
                call(went, C.byref(d), P(x), ldx, P(dy), lddy, P(dw), P(db), 0, P(ws), wsb, st)
                torch.cuda.synchronize()
                kinds = _timing_kinds(lib)
            finally:
                lib.of_timing_enable(0)
            assert kinds == [kind], "stage %d ran timing kinds %s" % (stage, kinds)
            assert torch.isfinite(dw).all() and torch.isfinite(db).all(), "stage %d" % stage
            out[stage] = (dw, db)
    finally:
        for k, v in DEFAULTS.items():
            lib.of_set_tuning(k, v)
    assert torch.equal(out[0][0], out[1][0]), "dw differs between the two stagings"
    assert torch.equal(out[0][1], out[1][1]), "db differs between the two stagings"
    # against an error common to both: the centre tap's dw against fp64, at the suite's REL_TOL
    xd, dyd = x[..., :cin].double().cpu(), dy[..., :cout].double().cpu()
    ref = torch.einsum("nhwi,nhwo->io", xd, dyd)
    assert rel_inf(out[1][0][1, 1], ref) < REL_TOL
