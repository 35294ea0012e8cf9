"""The 9-tap weight gradients' two x-halo stagings give bitwise the same sums.

conv_wgrad_tile_x3b / conv_wgrad_tile_b16 stage the x halo as one pixel-major image read with
transposing LDS reads, double-buffered (of_set_tuning key 40 = 1, the default); the _c3 kernels
keep the three pixel-shifted copies (key 40 = 0).  Both feed the same MFMA sequence with the
same operands, so dw and db must be torch.equal, not merely close.  Each case runs the weight
gradient through the C ABI with key 40 = 0 and = 1 into NaN-filled outputs, requires finite and
equal results and reads the timing kind to make sure the 9-tap kernel ran.

Shapes: the smallest at which the image can go wrong -- one whole tile; a shape smaller than a
tile (zero halo on all four sides); partial tiles and a partly empty second channel block;
slices of >= 4 tiles (the double buffer's prologue, steady state and last tile); every
instantiation's channel-block and wave shape (CIB 32 / 64, XH 8 / 4, MI 1 / 2); the one-plane
bf16 form.  One case has row strides larger than the channel counts, with NaN in the gaps.
"""
import ctypes as C
import zlib

import pytest
import torch

from helpers import REL_TOL, rel_inf, rng_tensor

pytestmark = pytest.mark.gpu

STAGE_KEY = 40
# of_set_tuning defaults of the keys the cases change (conv_f32.hip)
DEFAULTS = {4: 1, 5: 1, 13: 0, 33: 2, STAGE_KEY: 1}

# ((n, h, w, cin, cout), precision, {key: value}, timing kind, (ldx - cin_p, lddy - cout_p))
CASES = [
    ((1, 8, 16, 32, 128), "fp32", {}, 148, (0, 0)),            # one whole tile, one block
    ((1, 5, 7, 32, 128), "fp32", {}, 148, (0, 0)),             # zero halo on all four sides
    ((2, 9, 17, 40, 128), "fp32", {}, 148, (24, 12)),          # partial tiles, ragged block; strides
    ((3, 24, 32, 64, 256), "fp32", {33: 4}, 148, (0, 0)),      # slices of >= 4 tiles
    ((2, 16, 32, 96, 64), "fp32", {}, 152, (0, 0)),            # <2, 2, 8, 1>
    ((2, 16, 32, 64, 64), "fp32", {4: 2}, 150, (0, 0)),        # <4, 2, 4, 1>
    ((2, 16, 32, 128, 96), "fp32", {4: 2}, 149, (0, 0)),       # <2, 3, 8, 1>
    ((2, 16, 32, 64, 32), "fp32", {4: 2}, 151, (0, 0)),        # <4, 1, 4, 1>
    ((2, 9, 17, 40, 128), "fp32", {5: 2}, 148, (0, 0)),        # <1, 8, 8, 2>: two row blocks a wave
    ((2, 16, 32, 64, 64), "fp32", {4: 2, 5: 2}, 150, (0, 0)),  # <2, 4, 4, 2>
    ((2, 9, 17, 40, 128), "bf16", {13: 1}, 216, (0, 0)),       # conv_wgrad_tile_b16, one plane
    ((3, 24, 32, 64, 256), "bf16", {13: 1}, 216, (0, 0)),
]
_ID = lambda c: "x".join(map(str, c[0])) + "-" + c[1] + "".join("-k%d=%d" % kv for kv in c[2].items())


def _timing_kinds(lib):
    cap = 64
    k = (C.c_int * cap)()
    cnt = lib.of_timing_read(cap, k, None, None)
    assert cnt < cap
    return [k[i] for i in range(cnt)]


@pytest.mark.parametrize("case", CASES, ids=_ID)
def test_wgrad_stage_bitwise(case):
    from optical_flow_amd import _lib, ops
    from optical_flow_amd._lib import ACT_NONE, call
    (n, h, w, cin, cout), prec, keys, kind, (gx, gd) = case
    lib = _lib.lib()
    assert set(keys) <= set(DEFAULTS)
    seed = zlib.crc32(repr((n, h, w, cin, cout)).encode()) % 1000 + 500
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
        layer = ops.ConvLayer(wt, bias, stride=1, act=ACT_NONE, cin_p=cin_p, precision=prec,
                              f32_split=True)
        d = layer.desc(n, h, w)
        went, wsb = layer.wgrad_entry(d)
        assert went == ("of_conv2d_wgrad_bf16" if prec == "bf16" else "of_conv2d_wgrad_x3")
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
    # against an error common to both: the centre tap's dw against fp64.  fp32: the suite's
    # REL_TOL.  bf16: both operands rounded to 8 significand bits, |relative error| <= 2^-9
    # each and independent, so a sum of K unit-variance products is off by about 2^-9.3 sqrt(K)
    # (one standard deviation) while the largest of the cin x cout sums is about 3.7 sqrt(K):
    # 2^-8 of the largest sum is some nine standard deviations of the error.
    xd, dyd = x[..., :cin].double().cpu(), dy[..., :cout].double().cpu()
    ref = torch.einsum("nhwi,nhwo->io", xd, dyd)
    assert rel_inf(out[1][0][1, 1], ref) < (2.0 ** -8 if prec == "bf16" else REL_TOL)
