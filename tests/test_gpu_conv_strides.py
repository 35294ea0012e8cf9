"""The conv ABI's row strides (include/oflow.h: ldx, ldy, ldz, ldr, lddy, lddx, ld_act, ld_add,
ldt, ld_bn_res): every convolution entry point through the C ABI on channel slices of wider
NHWC buffers, the "virtual concat" the strides exist for.

Each case runs three stride variants on the same seeded data:

  contig  every stride is the channel count (the form every other test passes);
  concat  every tensor sits in a wider parent at a channel offset that is a multiple of 4,
          16-byte aligned, every stride a multiple of 4, no two strides of one call equal and
          none equal to a channel count of the layer;
  odd     x, dy and t as in concat (the header wants % 4 and 16-byte alignment for them), every
          other tensor with an odd stride at a one-channel offset (4-byte aligned pointers):
          the per-element epilogues.

Every tensor lives in a buffer of its own with a guard band before and behind its rows.  The
guards and the gap channels of an input hold a poison (1.0e4 or NaN), those of an output the
sentinel 7.0, and the output view itself starts as 7.0.  After the calls every element outside
a view must be bit for bit what it was (compared as int32), every output must be within REL_TOL
of the float64 oracle (on bf16-rounded operands for the bf16 entry points), the concat run must
have launched the kernels of the contig run (timing kinds) and must equal it bitwise; the odd
run's largest difference from contig is printed.

No family needed a "memory between rows must be finite" fallback: the NaN poison is
parametrised over every case, and bitwise equality with contig holds for every family.

Where an entry point documents a stricter rule the odd variant is left out or must be declined:
the Cout <= 4 input gradient (float4 rows), of_conv2d_b16i (% 4 strides: OF_EINVAL),
of_conv2d_fwd_pool and of_conv2d_dgrad_add_act_bnp (OF_EUNSUPPORTED, nothing written:
asserted).  One kernel choice depends on a stride: conv_stem_x3 has the float4 epilogue only,
so the odd variant's stem forward runs on the implicit GEMM (conv_fwd_impl: stem &&
vec_ep_ok); its difference from contig (4e-7) is the one nonzero figure the odd report prints.
"""
import ctypes as C
import zlib

import pytest
import torch

from helpers import REL_TOL, f64, rel_inf, rel_l2, rng_tensor
from oracle import ref_flow as R

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
ALPHA = 0.3
POISONS = [1.0e4, float("nan")]
ALIGNED = ("x", "dy", "t")           # GEMM A sources: ld % 4 == 0, 16-byte aligned pointer

KINDS_SEEN = {}                      # precision -> timing kinds, for the coverage report
RAN = set()
ODD_DIFF = {}                        # family -> largest |odd - contig| / max |contig|


def _ops():
    from optical_flow_amd import ops
    return ops


def _r4(c):
    return (c + 3) // 4 * 4


# ------------------------------------------------------------------ strided views ----
class _View:
    """npix rows of parent_channels floats between two guards; the view is channels
    [c0, c0 + c) of every row."""

    def __init__(self, parent_channels, c0, npix, c, fill, data=None, dtype=torch.float32):
        assert 0 <= c0 and c0 + c <= parent_channels
        guard = (max(256, parent_channels) + 7) // 8 * 8   # >= one row, >= 256, 16 bytes
        self.ld, self.c, self.npix = parent_channels, c, npix
        self.buf = torch.full((2 * guard + npix * parent_channels,), fill, device="cuda",
                              dtype=dtype)
        rows = self.buf[guard:guard + npix * parent_channels].view(npix, parent_channels)
        self.win = rows[:, c0:c0 + c]
        if data is None:                                 # an output: unwritten elements show
            self.win.fill_(SENTINEL)
        else:
            self.win.copy_(data.reshape(npix, c))
        self.ptr = self.buf.data_ptr() + self.buf.element_size() * (guard + c0)
        outside = torch.ones(self.buf.shape, dtype=torch.bool, device="cuda")
        outside[guard:guard + npix * parent_channels].view(npix, parent_channels)[:, c0:c0 + c] = False
        self._outside = outside
        self._bits = torch.int32 if dtype == torch.float32 else torch.int16
        self._snap = self.buf.view(self._bits).clone()

    def check(self, name, whole=False):
        """Guards and gaps (whole: the view too, for a pure input) are bitwise unchanged."""
        bad = self.buf.view(self._bits) != self._snap
        if not whole:
            bad &= self._outside
        nbad = int(bad.sum().item())
        if nbad:
            first = int(bad.nonzero()[0].item())
            raise AssertionError("%s: %d elements outside the view changed, first at flat index "
                                 "%d (ld %d, view of %d channels): %r" %
                                 (name, nbad, first, self.ld, self.c, self.buf[first].item()))

    def get(self, *shape):
        return self.win.clone().reshape(*shape, self.c)

    def __iter__(self):
        return iter((self.ptr, self.ld, self.check))


def view(parent_channels, c0, npix, c, fill, data=None, dtype=torch.float32):
    """One flat device buffer [guard | npix rows of parent_channels | guard]; returns the view's
    device pointer, its stride and a checker (iterable as that triple)."""
    return _View(parent_channels, c0, npix, c, fill, data, dtype)


_CONCAT_PAD = {"x": 8, "y": 20, "z": 4, "res": 12, "dy": 24, "t": 24, "act": 16, "add": 28,
               "dx": 36, "bn_res": 44, "y16": 8, "act16": 40}
_ODD_PAD = {"y": 1, "z": 3, "res": 5, "dx": 1, "act": 3, "add": 5, "bn_res": 7}


def layout(variant, chans, counts):
    """{name: (stride, channel offset)} for the tensors of ONE call (chans: name -> channels);
    counts: the layer's channel counts, which no concat / odd stride may equal."""
    taken = set(counts)
    out = {}
    for name, c in chans.items():
        if variant == "contig":
            out[name] = (c, 0)
            continue
        if variant == "odd" and name not in ALIGNED:
            ld = c + _ODD_PAD[name]
            ld += 1 - ld % 2
            while ld in taken:
                ld += 2
            c0 = 1
        else:
            ld = _r4(c) + _CONCAT_PAD[name] + (48 if variant == "odd" else 0)
            while ld in taken:
                ld += 32
            c0 = max(4, (ld - c) // 2 // 4 * 4)
            assert ld % 4 == 0 and c0 % 4 == 0
        assert ld > c and c0 + c <= ld
        taken.add(ld)
        out[name] = (ld, c0)
    if variant != "contig":
        lds = [v[0] for v in out.values()]
        assert len(set(lds)) == len(lds) and not set(lds) & set(counts), (out, counts)
    return out


def _views(variant, chans, counts, npix, fills, data):
    lay = layout(variant, chans, counts)
    return {k: view(lay[k][0], lay[k][1], npix[k], chans[k], fills[k], data.get(k)) for k in chans}


class _Timing:
    """Timing kinds of the conv launches inside the block."""

    def __init__(self, lib):
        self.lib, self.kinds = lib, set()

    def __enter__(self):
        self.lib.of_timing_read(0, None, None, None)       # drop earlier records
        self.lib.of_timing_enable(1)
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        cap = 256
        k = (C.c_int * cap)()
        cnt = self.lib.of_timing_read(cap, k, None, None)
        self.lib.of_timing_enable(0)
        assert cnt < cap
        self.kinds = {k[i] for i in range(cnt)}
        return False


# ------------------------------------------------------- which kernel a call selects ----
# Timing kinds (bench.py kind_parts) of one forward, input-gradient and weight-gradient call
# through the layer's own entry points, recorded before the host dispatch was rewritten as
# tables.  (n, h, w, cin, cout, k, stride), precision -> (fwd, dgrad, wgrad); None: not run.
DISPATCH_KINDS = {
    # (a) 3x3 stride 1 by N tile: conv_tile_x3 / conv_tile_bf16 BN 32 / 64 / 96 / 128 (at this
    # size key 27 gives the Cout 128 forward BN 64 tiles), weight-gradient configs 3 / 4 / 1 / 0
    # (Cout 64 from 32 input channels is config 4; from 64 it is config 2)
    ((1, 8, 32, 32, 32, 3, 1), "x3"): (131, 139, 147),
    ((1, 8, 32, 32, 32, 3, 1), "bf16"): (99, 107, 114),
    ((1, 8, 32, 32, 64, 3, 1), "x3"): (130, 139, 152),
    ((1, 8, 32, 64, 64, 3, 1), "x3"): (None, None, 146),
    ((1, 8, 32, 32, 64, 3, 1), "bf16"): (98, 107, 114),
    ((1, 8, 32, 32, 96, 3, 1), "x3"): (129, 139, 145),
    ((1, 8, 32, 32, 96, 3, 1), "bf16"): (97, 107, 112),
    ((1, 8, 32, 32, 128, 3, 1), "x3"): (130, 139, 148),
    ((1, 8, 32, 32, 128, 3, 1), "bf16"): (96, 107, 112),
    # (b) Cout 64 with Cin % 64 != 0: the 32 x 64 channel blocks, 9-tap form
    ((1, 8, 32, 96, 64, 3, 1), "x3"): (None, None, 152),
    # (c) the 8 x 32 output tiles need >= 4 workgroups per CU (x3_tall): "tall" / "flat" below
    ((8, 128, 256, 32, 128, 3, 1), "x3"): ({"tall": 128, "flat": 132}, None, None),
    ((8, 128, 256, 32, 128, 3, 1), "bf16"): ({"tall": 100, "flat": 96}, None, None),
    ((8, 16, 96, 128, 128, 3, 1), "x3"): (130, None, None),
    ((8, 16, 96, 128, 128, 3, 1), "bf16"): (96, None, None),
    # 1200 tiles of 4 x 32, unsplit: the single-buffered 4-wave BN 128 form
    ((2, 160, 480, 16, 128, 3, 1), "x3"): (132, None, None),
    # (d) stride 2: conv_gemm_x3 / conv_wgrad_x3 with three planes or one (key 16 = 6: bf16
    # forward on conv_gemm_bf16)
    ((1, 16, 16, 64, 128, 3, 2), "x3"): (160, 169, 176),
    ((1, 16, 16, 64, 128, 3, 2), "bf16"): (64, 249, 256),
    ((1, 16, 16, 64, 128, 1, 2), "x3"): (160, 169, 176),
    ((1, 16, 16, 64, 128, 1, 2), "bf16"): (64, 249, 256),
    ((1, 16, 16, 64, 64, 3, 2), "x3"): (161, 169, 177),
    ((1, 16, 16, 64, 64, 3, 2), "bf16"): (66, 249, 257),
    ((1, 16, 16, 64, 64, 1, 2), "x3"): (161, 169, 177),
    ((1, 16, 16, 64, 64, 1, 2), "bf16"): (66, 249, 257),
    # (e) the stem
    ((1, 32, 32, 3, 64, 7, 2), "x3"): (184, None, 185),
    ((1, 32, 32, 3, 64, 7, 2), "bf16"): (186, None, 187),
    # (f) Cout <= 4: the VALU kernels
    ((1, 8, 8, 32, 2, 3, 1), "f32"): (7, 15, 23),
}
# (g) one tuning key at a time on (a)'s Cout 128 layer: {precision: (fwd, dgrad, wgrad)}
DISPATCH_TUNED_SHAPE = (1, 8, 32, 32, 128, 3, 1)
DISPATCH_TUNED = {
    (40, 0): {"x3": (130, 139, 148), "bf16": (96, 107, 112)},
    (5, 2): {"x3": (130, 139, 148), "bf16": (96, 107, 112)},
    (4, 0): {"x3": (130, 139, 144), "bf16": (96, 107, 112)},
    (4, 2): {"x3": (130, 139, 148), "bf16": (96, 107, 112)},
    (12, 1): {"x3": (130, 139, 148), "bf16": (198, 203, 112)},
    (13, 1): {"x3": (130, 139, 148), "bf16": (96, 107, 216)},
    (36, 2): {"x3": (135, 139, 148), "bf16": (96, 107, 112)},
    (30, 0): {"x3": (130, 139, 148), "bf16": (96, 107, 112)},
    (30, 1): {"x3": (130, 139, 148), "bf16": (96, 107, 112)},
    (17, 0): {"x3": (130, 139, 148), "bf16": (96, 107, 112)},
    (20, 0): {"x3": (130, 139, 148), "bf16": (96, 107, 112)},
}
DISPATCH_BITWISE = {40, 30, 17, 20}      # keys that pick a sibling instance: the same bits
# key 30 picks among conv_gemm_x3 instances, which (a)'s layer never runs: (d)'s 3x3 too
DISPATCH_RING_SHAPE = (1, 16, 16, 64, 128, 3, 2)


def _dispatch_run(lib, shape, prec, passes=(0, 1, 2)):
    """One contiguous call per pass; ([kind or None] * 3, [output or None] * 3)."""
    from optical_flow_amd._lib import ACT_NONE, call
    ops = _ops()
    n, h, w, cin, cout, k, s = shape
    cin_p, cout_p = _r4(cin), _r4(cout)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(zlib.crc32(repr(shape).encode()))
    rnd = lambda *sh: torch.randn(*sh, device="cuda", generator=gen)
    layer = ops.ConvLayer(rnd(k, k, cin, cout) * (2.0 / (k * k * cin)) ** 0.5, rnd(cout) * 0.1,
                          stride=s, act=ACT_NONE, cin_p=cin_p,
                          precision="bf16" if prec == "bf16" else "fp32", f32_split=prec == "x3")
    d = layer.desc(n, h, w)
    wf, wd = layer.packed(d)
    x = torch.zeros(n, h, w, cin_p, device="cuda")
    x[..., :cin] = rnd(n, h, w, cin)
    dy = torch.zeros(n, d.ho, d.wo, cout_p, device="cuda")
    dy[..., :cout] = rnd(n, d.ho, d.wo, cout)
    P, st = ops._ptr, ops._stream()
    kinds, outs = [None] * 3, [None] * 3
    for m in passes:
        ent, wsb = (layer.fwd_entry, layer.dgrad_entry, layer.wgrad_entry)[m](d)
        ws = torch.empty(wsb // 4 + 4, device="cuda")
        with _Timing(lib) as tm:
            if m == 0:
                out = torch.full((n, d.ho, d.wo, cout), SENTINEL, device="cuda")
                call(ent, C.byref(d), P(x), cin_p, P(wf), P(layer.bias), None, None, None, None,
                     1e-3, None, 0, ACT_NONE, ALPHA, None, 0, P(out), cout, P(ws), wsb, st)
            elif m == 1:
                out = torch.full((n, h, w, cin_p), SENTINEL, device="cuda")
                call(ent, C.byref(d), P(dy), cout_p, P(wd), None, 0, ACT_NONE, ALPHA, P(out),
                     cin_p, P(ws), wsb, st)
            else:
                out = torch.full((k, k, cin, cout), SENTINEL, device="cuda")
                db = torch.full((cout,), SENTINEL, device="cuda")
                call(ent, C.byref(d), P(x), cin_p, P(dy), cout_p, P(out), P(db), 0, P(ws), wsb, st)
        assert len(tm.kinds) == 1, (shape, prec, m, tm.kinds)
        kinds[m], outs[m] = tm.kinds.pop(), out
    return kinds, outs


def _dispatch_measure(lib):
    """Everything test_dispatch_kinds compares: (kinds of DISPATCH_KINDS' calls, kinds per tuned
    key, the keys of DISPATCH_BITWISE whose outputs differed from the default run's)."""
    plain, tuned, differ = {}, {}, []
    base = {}
    for (shape, prec), want in DISPATCH_KINDS.items():
        passes = [m for m in range(3) if want[m] is not None]
        plain[shape, prec], outs = _dispatch_run(lib, shape, prec, passes)
        if shape == DISPATCH_TUNED_SHAPE:
            base[prec] = outs
    base["ring"] = _dispatch_run(lib, DISPATCH_RING_SHAPE, "x3")
    defaults = {40: 1, 5: 1, 4: 1, 12: 0, 13: 0, 36: 0, 30: 2, 17: 1, 20: 1}
    try:
        for (key, val) in DISPATCH_TUNED:
            assert lib.of_set_tuning(key, val) == 0
            tuned[key, val] = {}
            for prec in ("x3", "bf16"):
                tuned[key, val][prec], outs = _dispatch_run(lib, DISPATCH_TUNED_SHAPE, prec)
                if key in DISPATCH_BITWISE and not all(map(torch.equal, outs, base[prec])):
                    differ.append((key, val, prec))
            if key == 30:
                kinds, outs = _dispatch_run(lib, DISPATCH_RING_SHAPE, "x3")
                if kinds != base["ring"][0] or not all(map(torch.equal, outs, base["ring"][1])):
                    differ.append((key, val, "ring"))
            assert lib.of_set_tuning(key, defaults[key]) == 0
    finally:
        for key, val in defaults.items():
            lib.of_set_tuning(key, val)
    return plain, tuned, differ


def test_dispatch_kinds():
    """The kernel each call selects (its timing kind), by shape, precision and tuning key,
    against DISPATCH_KINDS / DISPATCH_TUNED; the sibling instances of keys 40, 30, 17 and 20
    give the default run's bits."""
    from optical_flow_amd import _lib
    lib = _lib.lib()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plain, tuned, differ = _dispatch_measure(lib)
    for (shape, prec), want in DISPATCH_KINDS.items():
        n, h, w = shape[:3]
        # x3_tall (conv_f32.hip): 8 x 32 tiles while they leave >= 4 workgroups per CU
        form = "tall" if n * -(-h // 8) * -(-w // 32) >= 4 * cus else "flat"
        want = [q[form] if isinstance(q, dict) else q for q in want]
        print("dispatch %s %s: %s" % ("x".join(map(str, shape)), prec, plain[shape, prec]))
        assert plain[shape, prec] == want, (shape, prec, plain[shape, prec], want)
    for setting, want in DISPATCH_TUNED.items():
        print("dispatch key %d = %d: %s" % (setting + (tuned[setting],)))
        assert tuned[setting] == {p: list(v) for p, v in want.items()}, (setting, tuned[setting])
    assert not differ, differ

# ------------------------------------------------------------------------- cases ----
# ((n, h, w, cin, cout, k, stride), forward activation, precisions)
CASES = [
    ((2, 16, 24, 16, 32, 3, 1), "leaky", ("x3", "bf16", "f32")),   # BN 32 tiles, wgrad cfg 3; f32 MFMA GEMM
    ((2, 20, 36, 64, 64, 3, 1), "relu", ("x3", "bf16")),           # BN 64, wgrad cfg 2 / 4
    ((2, 16, 16, 64, 96, 3, 1), "leaky", ("x3", "bf16")),          # BN 96
    ((2, 16, 24, 115, 128, 3, 1), "leaky", ("x3", "bf16")),        # decoder c0: partial chunk, 9-tap wgrad
    ((1, 13, 35, 48, 64, 3, 1), "leaky", ("bf16",)),               # ragged halo tiles, partial chunk
    ((1, 4, 8, 179, 128, 3, 1), "leaky", ("x3", "f32")),           # deep split-K: splitk_epilogue_kernel
    ((2, 48, 64, 256, 256, 3, 1), "relu", ("x3", "bf16")),         # K split: splitk_epilogue_flat
    ((1, 6, 10, 256, 44, 3, 1), "relu", ("x3",)),                  # N % 4 == 0, not a tile multiple
    ((1, 6, 10, 64, 42, 3, 1), "relu", ("x3",)),                   # N % 4 != 0
    ((1, 9, 9, 12, 2, 3, 1), "leaky", ("f32",)),                   # cin_p 12: GEMM fallback, cout 2
    ((1, 12, 16, 32, 2, 3, 1), "none", ("f32",)),                  # narrow VALU kernels, plain and
    ((2, 33, 70, 32, 2, 3, 1), "none", ("f32",)),                  # tiled, 1 to 16 lanes per pixel
    ((3, 40, 100, 32, 4, 3, 1), "leaky", ("f32",)),
    ((2, 17, 65, 32, 3, 3, 1), "none", ("f32",)),
    ((1, 10, 20, 64, 3, 3, 1), "relu", ("f32",)),
    ((2, 8, 8, 3, 2, 3, 1), "leaky", ("f32",)),
    ((2, 32, 48, 3, 64, 7, 2), "relu", ("x3", "bf16")),            # conv_stem_x3, conv_wgrad_stem_x3
    ((2, 16, 16, 64, 128, 3, 2), "relu", ("x3", "bf16", "f32")),   # stride-2 GEMM, 4 dgrad phase groups
    ((2, 16, 16, 64, 128, 1, 2), "none", ("x3", "bf16")),          # 1x1 / 2: empty phase groups
    ((3, 9, 7, 20, 40, 3, 2), "leaky", ("x3", "f32")),             # odd spatial size, stride 2
    # conv_tile_x3 takes BN = 128 tiles at default tuning only from 1200 workgroups up (key 27)
    ((2, 160, 480, 16, 128, 3, 1), "leaky", ("x3",)),
]
PARAMS = [(shape, act, prec) for shape, act, precs in CASES for prec in precs]
_ID = lambda p: "x".join(map(str, p[0])) + p[1] + "-" + p[2]

_DATA = {}
_ORACLE = {}


def _data(shape):
    """Seeded host tensors of one shape (shared by its precisions, poisons and variants)."""
    if shape in _DATA:
        return _DATA[shape]
    n, h, w, cin, cout, k, s = shape
    seed = zlib.crc32(repr(shape).encode()) % 1000 + 300
    ops = _ops()
    _, _, ho = ops.same_pads(h, k, s)
    _, _, wo = ops.same_pads(w, k, s)
    cin_p, cout_p = _r4(cin), _r4(cout)

    def padded(sh, c, cp, sd):
        t = torch.zeros(sh + (cp,))
        t[..., :c] = rng_tensor(sh + (c,), sd)
        return t

    dd = {
        "ho": ho, "wo": wo,
        "x": padded((n, h, w), cin, cin_p, seed),                       # [cin, cin_p) zero
        "w": rng_tensor((k, k, cin, cout), seed + 1, scale=(2.0 / (k * k * cin)) ** 0.5),
        "b": rng_tensor((cout,), seed + 2, scale=0.1),
        "g": rng_tensor((cout,), seed + 3, lo=0.5, hi=1.5),
        "be": rng_tensor((cout,), seed + 4, scale=0.1),
        "mu": rng_tensor((cout,), seed + 5, scale=0.1),
        "var": rng_tensor((cout,), seed + 6, lo=0.5, hi=1.5),
        "res": rng_tensor((n, ho, wo, cout), seed + 7),
        "dy": padded((n, ho, wo), cout, cout_p, seed + 8),              # [cout, cout_p) zero
        "act": rng_tensor((n, h, w, cin_p), seed + 9),
        "add": rng_tensor((n, h, w, cin_p), seed + 10),
        "dw0": rng_tensor((k, k, cin, cout), seed + 11, scale=0.1),
        "db0": rng_tensor((cout,), seed + 12, scale=0.1),
    }
    _DATA[shape] = dd
    return dd


def _oracle(shape, act, bf16):
    """float64 references, computed once per shape and operand rounding."""
    key = (shape, act, bf16)
    if key in _ORACLE:
        return _ORACLE[key]
    n, h, w, cin, cout, k, s = shape
    dd = _data(shape)
    assert R.CONV_PRECISION == "fp32" and abs(R.BN_EPS - 1e-3) < 1e-12
    xo, wo_, bo = [f64(t).requires_grad_(True) for t in (dd["x"][..., :cin], dd["w"], dd["b"])]
    g, be, mu, var = [f64(dd[q]) for q in ("g", "be", "mu", "var")]
    dy = f64(dd["dy"][..., :cout])
    if bf16:
        z = R._Bf16Conv.apply(xo, wo_, bo, s)
        bn = R._Bf16ConvBN.apply(xo.detach(), wo_.detach(), bo.detach(), g, be, mu, var, s)
    else:
        z = R.conv2d_same(xo, wo_, bo, s)
        bn = R.batchnorm_inference(z.detach(), {"bn/gamma": g, "bn/beta": be, "bn/moving_mean": mu,
                                                "bn/moving_variance": var}, "bn")
    (z * dy).sum().backward()
    fn = {"relu": torch.relu, "leaky": R.leaky_relu, "none": lambda t: t}[act]
    slope = torch.where(f64(dd["act"][..., :cin]) > 0, 1.0, ALPHA).double()
    o = {
        "z": z.detach(),
        "y": fn(bn + f64(dd["res"])),                    # bias, BN, residual, activation
        "y_plain": fn(z.detach()),                       # the narrow kernels: bias + activation
        "dx": xo.grad * slope,
        "dx_add": xo.grad + f64(dd["add"][..., :cin]),
        "dw": wo_.grad, "db": bo.grad,
        "dw_acc": wo_.grad + f64(dd["dw0"]), "db_acc": bo.grad + f64(dd["db0"]),
    }
    _ORACLE[key] = o
    return o


def _layer(shape, act, prec):
    from optical_flow_amd._lib import ACT_LEAKY, ACT_NONE, ACT_RELU
    ops = _ops()
    n, h, w, cin, cout, k, s = shape
    dd = _data(shape)
    code = {"relu": ACT_RELU, "leaky": ACT_LEAKY, "none": ACT_NONE}[act]
    layer = ops.ConvLayer(dd["w"].cuda(), dd["b"].cuda(), stride=s, act=code, cin_p=_r4(cin),
                          precision="bf16" if prec == "bf16" else "fp32",
                          f32_split=prec == "x3")
    return layer, code


def _run_variant(variant, shape, act, prec, poison, lib):
    """Every first-tier entry point of the layer's precision once; returns (outputs, kinds)."""
    from optical_flow_amd._lib import ACT_LEAKY, call
    ops = _ops()
    n, h, w, cin, cout, k, s = shape
    dd = _data(shape)
    ho, wo = dd["ho"], dd["wo"]
    cin_p, cout_p = _r4(cin), _r4(cout)
    counts = {cin, cin_p, cout, cout_p}
    npi, npo = n * h * w, n * ho * wo
    layer, act_code = _layer(shape, act, prec)
    d = layer.desc(n, h, w)
    narrow = lib.of_conv_path(C.byref(d)) == 1
    assert layer.mode(d) == {"x3": 2, "bf16": 1, "f32": 0}[prec] or (narrow and prec == "f32")
    wf, wd = layer.packed(d)
    fent, fws = layer.fwd_entry(d)
    dent, dws = layer.dgrad_entry(d)
    aent, aws = layer.dgrad_add_entry(d)
    went, wws = layer.wgrad_entry(d)
    if shape[:5] == (2, 48, 64, 256, 256):
        assert fws > 0 and dws > 0, "the K-split case must split K"
    ws = torch.empty(max(fws, dws, aws, wws) // 4 + 4, device="cuda")
    P, st = ops._ptr, ops._stream()
    dev = lambda q: dd[q].cuda()
    b, g, be, mu, var = [dev(q) for q in ("b", "g", "be", "mu", "var")]
    chk = []                                             # (view, name, whole)
    out = {}

    def mk(chans, npix, data):
        fills = {q: (poison if q in data else SENTINEL) for q in chans}
        v = _views(variant, chans, counts, npix, fills, data)
        for q in chans:
            chk.append((v[q], q, q in data))
        return v

    with _Timing(lib) as tm:
        # ---- forward: bias, BN, residual, z and the activation (narrow: bias + activation)
        if narrow:
            v = mk({"x": cin_p, "y": cout}, {"x": npi, "y": npo}, {"x": dd["x"]})
            call(fent, C.byref(d), v["x"].ptr, v["x"].ld, P(wf), P(b), None, None, None, None,
                 1e-3, None, 0, act_code, ALPHA, None, 0, v["y"].ptr, v["y"].ld, P(ws), fws, st)
        else:
            v = mk({"x": cin_p, "res": cout, "z": cout, "y": cout},
                   {"x": npi, "res": npo, "z": npo, "y": npo}, {"x": dd["x"], "res": dd["res"]})
            call(fent, C.byref(d), v["x"].ptr, v["x"].ld, P(wf), P(b), P(g), P(be), P(mu), P(var),
                 1e-3, v["res"].ptr, v["res"].ld, act_code, ALPHA, v["z"].ptr, v["z"].ld,
                 v["y"].ptr, v["y"].ld, P(ws), fws, st)
            out["z"] = v["z"]
        out["y"] = v["y"]
        # ---- input gradient with the activation derivative of act_src
        # (the Cout <= 4 kernels want float4 rows for dx and act_src: no odd variant, oflow.h)
        if not (narrow and variant == "odd"):
            v = mk({"dy": cout_p, "act": cin_p, "dx": cin_p}, {"dy": npo, "act": npi, "dx": npi},
                   {"dy": dd["dy"], "act": dd["act"]})
            call(dent, C.byref(d), v["dy"].ptr, v["dy"].ld, P(wd), v["act"].ptr, v["act"].ld,
                 ACT_LEAKY, ALPHA, v["dx"].ptr, v["dx"].ld, P(ws), dws, st)
            out["dx"] = v["dx"]
        if not narrow:                                   # (the Cout <= 4 kernels take no add)
            # ---- plus a separate added gradient, ld_add != lddx
            v = mk({"dy": cout_p, "add": cin_p, "dx": cin_p}, {"dy": npo, "add": npi, "dx": npi},
                   {"dy": dd["dy"], "add": dd["add"]})
            if variant != "contig":
                assert v["add"].ld != v["dx"].ld
            call(aent, C.byref(d), v["dy"].ptr, v["dy"].ld, P(wd), v["add"].ptr, v["add"].ld,
                 v["dx"].ptr, v["dx"].ld, P(ws), aws, st)
            out["dx_add"] = v["dx"]
            # ---- in place: add == dx (1x1 stride 2: only the phase group a tap reaches runs)
            lay = layout(variant, {"dy": cout_p, "dx": cin_p}, counts)
            vdy = view(lay["dy"][0], lay["dy"][1], npo, cout_p, poison, dd["dy"])
            vdx = view(lay["dx"][0], lay["dx"][1], npi, cin_p, SENTINEL, dd["add"])
            chk += [(vdy, "dy", True), (vdx, "dx in place", False)]
            call(aent, C.byref(d), vdy.ptr, vdy.ld, P(wd), vdx.ptr, vdx.ld, vdx.ptr, vdx.ld,
                 P(ws), aws, st)
            out["dx_inplace"] = vdx
        # ---- weight and bias gradient, written and accumulated
        dws_out = {}
        for acc in (0, 1):
            v = mk({"x": cin_p, "dy": cout_p}, {"x": npi, "dy": npo},
                   {"x": dd["x"], "dy": dd["dy"]})
            dw = dev("dw0") if acc else torch.full((k, k, cin, cout), SENTINEL, device="cuda")
            db = dev("db0") if acc else torch.full((cout,), SENTINEL, device="cuda")
            call(went, C.byref(d), v["x"].ptr, v["x"].ld, v["dy"].ptr, v["dy"].ld, P(dw), P(db),
                 acc, P(ws), wws, st)
            dws_out["dw_acc" if acc else "dw"] = dw
            dws_out["db_acc" if acc else "db"] = db
    for vw, name, whole in chk:
        vw.check("%s %s" % (variant, name), whole)
    res = {"y": out["y"].get(n, ho, wo)}
    if "z" in out:
        res["z"] = out["z"].get(n, ho, wo)
    for q in ("dx", "dx_add", "dx_inplace"):
        if q in out:
            res[q] = out[q].get(n, h, w)
    res.update(dws_out)
    return res, tm.kinds, narrow


def _families(kinds):
    from bench import kind_parts
    return {kind_parts(q) for q in kinds}


def _assert_family(shape, prec, narrow, kinds):
    """The kernels the case is in the table for ran (bench.py kind_parts)."""
    from bench import X3_BN
    n, h, w, cin, cout, k, s = shape
    parts = _families(kinds)
    fams = {(m, f) for m, _, f in parts}
    if narrow:
        assert {(0, 7, "f32"), (1, 7, "f32"), (2, 7, "f32")} <= parts, parts
    elif (k, s) == (7, 2):
        assert ({184, 185} if prec == "x3" else {186, 187}) <= kinds, kinds
    elif prec == "f32":
        assert {(0, "f32"), (1, "f32")} <= fams and all(c != 7 for _, c, _ in parts), parts
    elif (k, s) == (3, 1):
        fam = "tile_x3" if prec == "x3" else "tile_bf16"
        assert {(0, fam), (1, fam)} <= fams, parts
        if cout in (32, 64, 96) or cout % 128 == 0:      # (wgx3_cfg: the tiled weight gradients)
            assert (2, fam) in fams, parts
        if prec == "x3" and cout in (32, 64, 96):
            assert {X3_BN[c].split(",")[0] for m, c, f in parts if m == 0} == {str(cout)}, parts
        if shape[:3] == (2, 160, 480):
            assert {X3_BN[c].split(",")[0] for m, c, f in parts if m == 0} == {"128"}, parts
    elif prec == "x3":
        assert {(0, "gemm_x3"), (1, "gemm_x3"), (2, "gemm_x3")} <= fams, parts
    else:                      # bf16 implicit GEMMs: key 16 = 6, dgrad / wgrad on the one-plane form
        assert {(0, "bf16"), (1, "gemm_b16"), (2, "gemm_b16")} <= fams, parts


@pytest.mark.parametrize("poison", POISONS, ids=["1e4", "nan"])
@pytest.mark.parametrize("shape,act,prec", PARAMS, ids=[_ID(p) for p in PARAMS])
def test_conv_strides(shape, act, prec, poison):
    """of_conv2d_{fwd,dgrad,dgrad_add,wgrad}{,_x3,_bf16} in the three stride variants (module
    docstring): oracle bound, untouched gaps and guards, the same kernels and the same bits in
    the concat run as in the contiguous one, zero gradient in the pad channels."""
    from optical_flow_amd import _lib
    lib = _lib.lib()
    n, h, w, cin, cout, k, s = shape
    cin_p = _r4(cin)
    dd = _data(shape)
    ref = _oracle(shape, act, prec == "bf16")
    runs = {}
    for variant in ("contig", "concat", "odd"):
        runs[variant] = _run_variant(variant, shape, act, prec, poison, lib)
    narrow = runs["contig"][2]
    for variant, (res, kinds, _) in runs.items():
        for q, got in res.items():
            if q in ("dw", "db", "dw_acc", "db_acc"):
                err = rel_l2(got, ref[q])
            elif q in ("dx", "dx_add", "dx_inplace"):
                err = rel_inf(got[..., :cin], ref["dx" if q == "dx" else "dx_add"])
            else:
                err = rel_inf(got, ref["y_plain"] if (q == "y" and narrow) else ref[q])
            assert err < REL_TOL, (variant, q, err)
        if cin < cin_p:
            if "dx" in res:
                assert res["dx"][..., cin:].abs().max().item() == 0.0, (variant, "pad channels")
            for q in ("dx_add", "dx_inplace"):
                if q in res:       # 0 + add
                    assert torch.equal(res[q][..., cin:], dd["add"][..., cin:].cuda()), (variant, q)
    base, kinds0, _ = runs["contig"]
    _assert_family(shape, prec, narrow, kinds0)
    assert runs["concat"][1] == kinds0, ("concat ran other kernels", runs["concat"][1], kinds0)
    for q, got in runs["concat"][0].items():
        assert torch.equal(got, base[q]), ("concat != contig", q, rel_inf(got, base[q]))
    fam = "%s %s" % (prec, "narrow" if narrow else "%dx%d/%d" % (k, k, s))
    worst = 0.0
    for q, got in runs["odd"][0].items():
        worst = max(worst, rel_inf(got, base[q]))
    print("odd vs contig %s %s: %.2e" % (_ID((shape, act, prec)), sorted(runs["odd"][1]), worst))
    ODD_DIFF[fam] = max(ODD_DIFF.get(fam, 0.0), worst)
    KINDS_SEEN.setdefault(prec, set()).update(kinds0)     # (= the concat run's)
    RAN.add((shape, prec))


# ------------------------------------------------- second tier: the fused entry points ----
def _compare(runs, label):
    """concat ran the kernels of contig and equals it bitwise; odd (if run): report."""
    base, kinds0 = runs["contig"]
    res, kinds = runs["concat"]
    assert kinds == kinds0, (label, "concat ran other kernels", kinds, kinds0)
    for q, got in res.items():
        assert torch.equal(got, base[q]), (label, "concat != contig", q, rel_inf(got, base[q]))
    if runs.get("odd"):
        worst = max(rel_inf(got, base[q]) for q, got in runs["odd"][0].items())
        print("odd vs contig %s %s: %.2e" % (label, sorted(runs["odd"][1]), worst))
        ODD_DIFF[label] = max(ODD_DIFF.get(label, 0.0), worst)


def _check_all(chk, variant):
    for vw, name, whole in chk:
        vw.check("%s %s" % (variant, name), whole)


def _mk(variant, chans, counts, npix, data, poison, chk):
    fills = {q: (poison if q in data else SENTINEL) for q in chans}
    v = _views(variant, chans, counts, npix, fills, data)
    chk += [(v[q], q, q in data) for q in chans]
    return v


@pytest.mark.parametrize("poison", POISONS, ids=["1e4", "nan"])
def test_dgrad_add_act_strides(poison):
    """of_conv2d_dgrad_add_act (dx = act'(act_src) * (dgrad(dy) + add), the derivative after the
    sum) at the shape of test_dgrad_add_in_place on the split 3x3 tiles, with ld_add, ld_act
    and lddx all different, and in place (add == dx)."""
    from optical_flow_amd import _lib
    from optical_flow_amd._lib import ACT_LEAKY, ACT_NONE, call
    ops, lib = _ops(), _lib.lib()
    n, h, w, cin, cout, k, s = 2, 16, 20, 64, 128, 3, 1
    wt = rng_tensor((k, k, cin, cout), 7, scale=0.1)
    layer = ops.ConvLayer(wt.cuda(), rng_tensor((cout,), 8).cuda(), stride=s, act=ACT_NONE,
                          cin_p=cin, f32_split=True)
    d = layer.desc(n, h, w)
    assert layer.mode(d) == 2
    _, wd = layer.packed(d)
    dy = rng_tensor((n, h, w, cout), 9)
    add = rng_tensor((n, h, w, cin), 10)
    src = rng_tensor((n, h, w, cin), 11)
    xo = torch.zeros(n, h, w, cin, dtype=torch.float64, requires_grad=True)
    (R.conv2d_same(xo, f64(wt), None, s) * f64(dy)).sum().backward()
    ref = (xo.grad + f64(add)) * torch.where(f64(src) > 0, 1.0, ALPHA)
    _, wsz = layer.dgrad_add_entry(d)
    ws = torch.empty(wsz // 4 + 4, device="cuda")
    P, st = ops._ptr, ops._stream()
    npix, counts = n * h * w, {cin, cout}
    runs = {}
    for variant in ("contig", "concat", "odd"):
        chk = []
        with _Timing(lib) as tm:
            v = _mk(variant, {"dy": cout, "add": cin, "act": cin, "dx": cin}, counts,
                    dict.fromkeys(("dy", "add", "act", "dx"), npix),
                    {"dy": dy, "add": add, "act": src}, poison, chk)
            call("of_conv2d_dgrad_add_act", C.byref(d), 2, v["dy"].ptr, v["dy"].ld, P(wd),
                 v["add"].ptr, v["add"].ld, v["act"].ptr, v["act"].ld, ACT_LEAKY, ALPHA,
                 v["dx"].ptr, v["dx"].ld, P(ws), wsz, st)
            lay = layout(variant, {"dy": cout, "act": cin, "dx": cin}, counts)
            u = {"dy": view(*lay["dy"], npix, cout, poison, dy),
                 "act": view(*lay["act"], npix, cin, poison, src),
                 "dx": view(*lay["dx"], npix, cin, SENTINEL, add)}
            chk += [(u["dy"], "dy", True), (u["act"], "act", True), (u["dx"], "dx in place", False)]
            call("of_conv2d_dgrad_add_act", C.byref(d), 2, u["dy"].ptr, u["dy"].ld, P(wd),
                 u["dx"].ptr, u["dx"].ld, u["act"].ptr, u["act"].ld, ACT_LEAKY, ALPHA,
                 u["dx"].ptr, u["dx"].ld, P(ws), wsz, st)
        _check_all(chk, variant)
        res = {"dx": v["dx"].get(n, h, w), "dx_inplace": u["dx"].get(n, h, w)}
        for q, got in res.items():
            assert rel_inf(got, ref) < REL_TOL, (variant, q)
        runs[variant] = (res, tm.kinds)
    assert {(1, "tile_x3")} <= {(m, f) for m, _, f in _families(runs["contig"][1])}
    _compare(runs, "dgrad_add_act x3")


@pytest.mark.parametrize("poison", POISONS, ids=["1e4", "nan"])
def test_wgrad_bn_strides(poison):
    """of_conv2d_wgrad_bn (dw = s * (x^T t), s = gamma / sqrt(var + eps)) with ldx and ldt
    strided, at a test_conv_x3_bn64_forms shape."""
    from optical_flow_amd import _lib
    from optical_flow_amd._lib import ACT_NONE, call
    ops, lib = _ops(), _lib.lib()
    n, h, w, cin, cout = 2, 37, 45, 64, 64
    x = rng_tensor((n, h, w, cin), 121)
    wt = rng_tensor((3, 3, cin, cout), 122, scale=(2.0 / (9 * cin)) ** 0.5)
    t = rng_tensor((n, h, w, cout), 123)
    gamma = rng_tensor((cout,), 124, lo=0.5, hi=1.5)
    var = rng_tensor((cout,), 125, lo=0.5, hi=1.5)
    layer = ops.ConvLayer(wt.cuda(), torch.zeros(cout).cuda(), stride=1, act=ACT_NONE, cin_p=cin,
                          f32_split=True)
    d = layer.desc(n, h, w)
    wo_ = f64(wt).requires_grad_(True)
    (R.conv2d_same(f64(x), wo_, None, 1) * f64(t)).sum().backward()
    ref = wo_.grad * (f64(gamma) / torch.sqrt(f64(var) + 1e-3))
    wsb = lib.of_conv2d_wgrad_bn_workspace(C.byref(d), 2)
    ws = torch.empty(wsb // 4 + 4, device="cuda")
    P, st = ops._ptr, ops._stream()
    gd, vd = gamma.cuda(), var.cuda()
    npix = n * h * w
    runs = {}
    for variant in ("contig", "concat", "odd"):
        chk = []
        with _Timing(lib) as tm:
            v = _mk(variant, {"x": cin, "t": cout}, {cin, cout}, {"x": npix, "t": npix},
                    {"x": x, "t": t}, poison, chk)
            assert variant == "contig" or v["x"].ld != v["t"].ld
            dw = torch.full((3, 3, cin, cout), SENTINEL, device="cuda")
            call("of_conv2d_wgrad_bn", C.byref(d), 2, v["x"].ptr, v["x"].ld, v["t"].ptr,
                 v["t"].ld, P(dw), 0, P(gd), P(vd), 1e-3, P(ws), wsb, st)
        _check_all(chk, variant)
        assert rel_l2(dw, ref) < REL_TOL, variant
        runs[variant] = ({"dw": dw}, tm.kinds)
    assert {(2, "tile_x3")} <= {(m, f) for m, _, f in _families(runs["contig"][1])}
    _compare(runs, "wgrad_bn x3")


@pytest.mark.parametrize("poison", POISONS, ids=["1e4", "nan"])
def test_dgrad_bnp_strides(poison):
    """of_conv2d_dgrad_add_act_bnp at the one-slice shape of test_dgrad_bnp_partials with
    lddy, ld_add, ld_act, lddx and ld_bn_res all different: dx against the oracle, dx and the BN
    partial sums bitwise those of the contiguous call.  The partial sums ride on the 16-byte
    epilogue only: odd strides are declined with OF_EUNSUPPORTED and nothing is written."""
    from optical_flow_amd import _lib
    from optical_flow_amd._lib import ACT_RELU, OF_EUNSUPPORTED
    ops, lib = _ops(), _lib.lib()
    n, h, w, cin, cout = 8, 96, 128, 64, 64
    wt = rng_tensor((3, 3, cin, cout), 71, scale=(2.0 / (9 * cin)) ** 0.5)
    layer = ops.ConvLayer(wt.cuda(), rng_tensor((cout,), 72, scale=0.1).cuda(), stride=1,
                          act=ACT_RELU, cin_p=cin, f32_split=True)
    d = layer.desc(n, h, w)
    _, wd = layer.packed(d)
    dy = rng_tensor((n, h, w, cout), 73)
    y = torch.relu(rng_tensor((n, h, w, cin), 74))                 # the BN layer's output
    add = rng_tensor((n, h, w, cin), 75)
    rres = rng_tensor((n, h, w, cin), 79)
    gamma = (rng_tensor((cin,), 76, scale=0.5) + 1.0).cuda()
    beta = rng_tensor((cin,), 77, scale=0.2).cuda()
    key = "bnp"
    if key not in _ORACLE:
        xo = torch.zeros(n, h, w, cin, dtype=torch.float64, requires_grad=True)
        (R.conv2d_same(xo, f64(wt), None, 1) * f64(dy)).sum().backward()
        _ORACLE[key] = (xo.grad + f64(add)) * (f64(y) > 0)
    ref = _ORACLE[key]
    _, wsz = layer.dgrad_add_entry(d)
    ws = torch.empty(max(wsz, 4) // 4 + 4, device="cuda")
    pb = lib.of_conv2d_dgrad_bnp_bytes(C.byref(d))
    assert pb > 0
    P, st = ops._ptr, ops._stream()
    npix = n * h * w
    names = ("dy", "add", "act", "bn_res", "dx")
    runs = {}
    for variant in ("contig", "concat", "odd"):
        chk = []
        part = torch.full((pb // 4 + 4,), SENTINEL, device="cuda")
        nblk = C.c_int(0)
        with _Timing(lib) as tm:
            v = _mk(variant, dict(dy=cout, add=cin, act=cin, bn_res=cin, dx=cin), {cin, cout},
                    dict.fromkeys(names, npix), {"dy": dy, "add": add, "act": y, "bn_res": rres},
                    poison, chk)
            rc = lib.of_conv2d_dgrad_add_act_bnp(
                C.byref(d), 2, v["dy"].ptr, v["dy"].ld, P(wd), v["add"].ptr, v["add"].ld,
                v["act"].ptr, v["act"].ld, ACT_RELU, C.c_float(0.0), v["dx"].ptr, v["dx"].ld,
                P(gamma), P(beta), v["bn_res"].ptr, v["bn_res"].ld, P(part), pb, C.byref(nblk),
                P(ws), wsz, st)
        _check_all(chk, variant)
        dx = v["dx"].get(n, h, w)
        if variant == "odd":
            assert rc == OF_EUNSUPPORTED, (rc, lib.of_last_error())
            assert tm.kinds == set()
            assert (dx == SENTINEL).all() and (part == SENTINEL).all(), "declined, yet written"
            continue
        assert rc == 0, lib.of_last_error()
        assert nblk.value > 0
        assert rel_inf(dx, ref) < REL_TOL, variant
        runs[variant] = ({"dx": dx, "part": part[:nblk.value * 2 * cin].clone()}, tm.kinds)
    assert {(1, "tile_x3")} <= {(m, f) for m, _, f in _families(runs["contig"][1])}
    _compare(runs, "dgrad_add_act_bnp x3")


@pytest.mark.parametrize("poison", POISONS, ids=["1e4", "nan"])
def test_fwd_pool_strides(poison):
    """of_conv2d_fwd_pool (the stem forward with the 2x2 max-pool in its epilogue) with ldy and
    ldz strided: y and z against the oracle, pool bit-identical to of_maxpool2_fwd of the
    strided y.  The stem kernel stores float4 columns: odd strides are declined with
    OF_EUNSUPPORTED and nothing is written."""
    from optical_flow_amd import _lib
    from optical_flow_amd._lib import ACT_RELU, OF_EUNSUPPORTED, call
    ops, lib = _ops(), _lib.lib()
    n, h, w, cin, cout, k, s = 4, 64, 128, 3, 64, 7, 2
    x = torch.zeros(n, h, w, 4)
    x[..., :cin] = rng_tensor((n, h, w, cin), 201)
    wt = rng_tensor((k, k, cin, cout), 202, scale=(2.0 / (k * k * cin)) ** 0.5)
    b, g, be, mu, var = (rng_tensor((cout,), 203, scale=0.1), rng_tensor((cout,), 204, lo=0.5, hi=1.5),
                         rng_tensor((cout,), 205, scale=0.1), rng_tensor((cout,), 206, scale=0.1),
                         rng_tensor((cout,), 207, lo=0.5, hi=1.5))
    layer = ops.ConvLayer(wt.cuda(), b.cuda(), stride=s, act=ACT_RELU, cin_p=4, f32_split=True)
    d = layer.desc(n, h, w)
    assert layer.mode(d) == 2
    wf, _ = layer.packed(d)
    ho, wo = d.ho, d.wo
    zo = R.conv2d_same(f64(x[..., :cin]), f64(wt), f64(b), s)
    yo = torch.relu(R.batchnorm_inference(zo, {"bn/gamma": f64(g), "bn/beta": f64(be),
                                               "bn/moving_mean": f64(mu),
                                               "bn/moving_variance": f64(var)}, "bn"))
    fws = lib.of_conv2d_fwd_x3_workspace(C.byref(d))
    ws = torch.empty(fws // 4 + 4, device="cuda")
    P, st = ops._ptr, ops._stream()
    bd, gd, bed, mud, vard = [q.cuda() for q in (b, g, be, mu, var)]
    npi, npo = n * h * w, n * ho * wo
    runs = {}
    for variant in ("contig", "concat", "odd"):
        chk = []
        pool = torch.full((n, ho // 2, wo // 2, cout), SENTINEL, device="cuda")
        with _Timing(lib) as tm:
            v = _mk(variant, {"x": 4, "z": cout, "y": cout}, {cin, 4, cout},
                    {"x": npi, "z": npo, "y": npo}, {"x": x}, poison, chk)
            rc = lib.of_conv2d_fwd_pool(
                C.byref(d), 2, v["x"].ptr, v["x"].ld, P(wf), P(bd), P(gd), P(bed), P(mud), P(vard),
                C.c_float(1e-3), ACT_RELU, C.c_float(0.0), v["z"].ptr, v["z"].ld, v["y"].ptr,
                v["y"].ld, P(pool), P(ws), fws, st)
        _check_all(chk, variant)
        yd, zd = v["y"].get(n, ho, wo), v["z"].get(n, ho, wo)
        if variant == "odd":
            assert rc == OF_EUNSUPPORTED, (rc, lib.of_last_error())
            assert tm.kinds == set()
            assert (yd == SENTINEL).all() and (zd == SENTINEL).all() and (pool == SENTINEL).all()
            continue
        assert rc == 0, lib.of_last_error()
        assert rel_inf(yd, yo) < REL_TOL and rel_inf(zd, zo) < REL_TOL, variant
        pool2 = torch.full_like(pool, SENTINEL)
        call("of_maxpool2_fwd", P(yd), n, ho, wo, cout, P(pool2), st)
        torch.cuda.synchronize()
        assert torch.equal(pool, pool2), variant
        runs[variant] = ({"y": yd, "z": zd, "pool": pool}, tm.kinds)
    assert 184 in runs["contig"][1]
    _compare(runs, "fwd_pool x3")


@pytest.mark.parametrize("poison", POISONS, ids=["1e4", "nan"])
def test_b16i_strides(poison):
    """of_conv2d_b16i, forward and input gradient, at the padded-channel case of B16I_CASES with
    ldy, ldy16, ld_act and ld_act16 wider than the channel count (the entry point wants % 4
    strides and aligned pointers for all of them: no odd variant): fp32 and bf16-image outputs
    against float64 convolutions of the bf16-rounded operands, bitwise the contiguous call's."""
    import torch.nn.functional as Fn
    from optical_flow_amd import _lib
    from optical_flow_amd._lib import ACT_LEAKY, B16iIO, ConvDesc, call
    ops, lib = _ops(), _lib.lib()
    P, st = ops._ptr, ops._stream()
    n, h, w, cin, cout = 3, 17, 33, 115, 128
    seed = zlib.crc32(repr((n, h, w, cin, cout)).encode()) % 1000
    cin_p, cout_p = _r4(cin), _r4(cout)
    lx, ly = (cin_p + 31) // 32 * 32, (cout_p + 31) // 32 * 32
    d = ConvDesc(n, h, w, cin, cin_p, cout, 3, 3, 1, 1, 1, h, w)
    bf = lambda q: f64(q.to(torch.bfloat16).float())
    nchw = lambda q: q.permute(0, 3, 1, 2)
    nhwc = lambda q: q.permute(0, 2, 3, 1)
    x = rng_tensor((n, h, w, cin), seed)
    wt = rng_tensor((3, 3, cin, cout), seed + 1, scale=(2.0 / (9 * cin)) ** 0.5)
    bias = rng_tensor((cout,), seed + 2, scale=0.1)
    dy = rng_tensor((n, h, w, cout), seed + 3)
    src = torch.zeros(n, h, w, cin_p)
    src[..., :cin] = rng_tensor((n, h, w, cin), seed + 4)
    wk = bf(wt).permute(3, 2, 0, 1).contiguous()
    y_o = nhwc(Fn.conv2d(nchw(bf(x)), wk, f64(bias), padding=1))
    y_o = torch.where(y_o > 0, y_o, 0.3 * y_o)
    slope = torch.where(f64(src[..., :cin]) > 0, 1.0, 0.3).double()
    dx_o = nhwc(torch.nn.grad.conv2d_input((n, cin, h, w), wk, nchw(bf(dy)), padding=1)) * slope

    def img16(q, c, ld):
        o = torch.zeros(q.numel() // q.shape[-1] * ld, dtype=torch.bfloat16, device="cuda")
        call("of_to_bf16_image", P(q), q.numel() // q.shape[-1], c, q.shape[-1], P(o), ld, st)
        return o

    def io(**kw):
        r = B16iIO()
        for q, val in kw.items():
            setattr(r, q, val)
        return r

    wf = torch.empty(lib.of_conv_wfwd16_elems(C.byref(d)), dtype=torch.bfloat16, device="cuda")
    wb = torch.empty(lib.of_conv_wbwd16_elems(C.byref(d)), dtype=torch.bfloat16, device="cuda")
    call("of_conv_pack_weights_bf16", C.byref(d), P(wt.cuda()), P(wf), P(wb), st)
    xd = torch.zeros(n, h, w, cin_p, device="cuda")
    xd[..., :cin] = x.cuda()
    dyd = torch.zeros(n, h, w, cout_p, device="cuda")
    dyd[..., :cout] = dy.cuda()
    x16, dy16 = img16(xd, cin_p, lx), img16(dyd, cout_p, ly)
    bd = bias.cuda()
    npix = n * h * w
    B16 = torch.bfloat16
    runs = {}
    for variant in ("contig", "concat"):
        lay = layout(variant, {"y": cout, "y16": cout, "act": cin_p, "act16": cin_p, "dx": cin_p,
                               "dy": cin_p},     # ("dy": one more % 4 stride, for dx16)
                     {cin, cin_p, cout, lx, ly})
        vy = view(*lay["y"], npix, cout, SENTINEL)
        vy16 = view(*lay["y16"], npix, cout, SENTINEL, dtype=B16)
        vact = view(*lay["act"], npix, cin_p, poison, src)
        vact16 = view(*lay["act16"], npix, cin_p, poison, src.bfloat16(), dtype=B16)
        vdx = view(*lay["dx"], npix, cin_p, SENTINEL)
        vdx16 = view(*lay["dy"], npix, cin_p, SENTINEL, dtype=B16)
        chk = [(vy, "y", False), (vy16, "y16", False), (vact, "act_src", True),
               (vact16, "act16", True), (vdx, "dx", False), (vdx16, "dx16", False)]
        with _Timing(lib) as tm:
            for o in (io(a16=x16.data_ptr(), lda16=lx, y=vy.ptr, ldy=vy.ld),
                      io(a16=x16.data_ptr(), lda16=lx, y16=vy16.ptr, ldy16=vy16.ld)):
                call("of_conv2d_b16i", 0, C.byref(d), C.byref(o), P(wf), P(bd), None, None, None,
                     None, 0.0, ACT_LEAKY, 0.3, st)
            for o in (io(a16=dy16.data_ptr(), lda16=ly, y=vdx.ptr, ldy=vdx.ld, act_src=vact.ptr,
                         ld_act=vact.ld),
                      io(a16=dy16.data_ptr(), lda16=ly, y16=vdx16.ptr, ldy16=vdx16.ld,
                         act16=vact16.ptr, ld_act16=vact16.ld)):
                call("of_conv2d_b16i", 1, C.byref(d), C.byref(o), P(wb), None, None, None, None,
                     None, 0.0, ACT_LEAKY, 0.3, st)
        _check_all(chk, variant)
        res = {"y": vy.get(n, h, w), "y16": vy16.get(n, h, w), "dx": vdx.get(n, h, w),
               "dx16": vdx16.get(n, h, w)}
        tol = 1e-4                     # same bf16 operands: fp32 summation order only
        assert rel_inf(res["y"], y_o) < tol, variant
        assert torch.equal(res["y16"], res["y"].bfloat16()), variant
        assert rel_inf(res["dx"][..., :cin], dx_o) < tol, variant
        assert cin < cin_p and res["dx"][..., cin:].abs().max().item() == 0.0, variant
        assert torch.equal(res["dx16"], res["dx"].bfloat16()), variant
        runs[variant] = (res, tm.kinds)
    assert all(q >= 288 for q in runs["contig"][1]) and runs["contig"][1]
    _compare(runs, "b16i")


def test_kind_coverage():
    """The union of the timing kinds the first-tier cases launched, printed once; after a full
    run of this module it covers every conv family default tuning selects."""
    from bench import X3_BN, kind_parts
    for prec in sorted(KINDS_SEEN):
        print("timing kinds %s: %s" % (prec, sorted(KINDS_SEEN[prec])))
        print("   ", sorted({kind_parts(q) for q in KINDS_SEEN[prec]}))
    for fam in sorted(ODD_DIFF):
        print("odd vs contig, largest relative difference, %s: %.2e" % (fam, ODD_DIFF[fam]))
    if RAN != {(p[0], p[2]) for p in PARAMS}:
        return                                     # a partial selection (-k): report only
    f32 = {kind_parts(q) for q in KINDS_SEEN["f32"]}
    x3 = {kind_parts(q) for q in KINDS_SEEN["x3"]}
    b16 = {kind_parts(q) for q in KINDS_SEEN["bf16"]}
    for m in (0, 1, 2):
        assert (m, 7, "f32") in f32, ("narrow", m)
        assert any(p[0] == m and p[1] != 7 and p[2] in ("f32", "tile_f32") for p in f32), ("f32 GEMM", m)
        assert any(p[0] == m and p[2] == "gemm_x3" for p in x3), ("gemm_x3", m)
        assert any(p[0] == m and p[2] == "tile_bf16" for p in b16), ("tile_bf16", m)
    assert {X3_BN[c].split(",")[0] for m, c, f in x3 if f == "tile_x3" and m == 0} >= \
        {"32", "64", "96", "128"}, x3
    assert {184, 185} <= KINDS_SEEN["x3"] and {186, 187} <= KINDS_SEEN["bf16"]
    assert any(p[2] in ("bf16", "gemm_b16") and p[0] == 0 for p in b16)
    assert any(p[2] == "gemm_b16" and p[0] == 1 for p in b16)
    assert any(p[2] == "gemm_b16" and p[0] == 2 for p in b16)
    wg = {q for q in KINDS_SEEN["x3"] if 144 <= q < 160}
    assert any(q < 148 for q in wg) and any(q >= 148 for q in wg), ("3-tap and 9-tap wgrad", wg)
