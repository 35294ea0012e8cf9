"""Host side of the KITTI flow evaluation: the 16-bit PNG decode and encode against an
independent codec (tests/kitti_flow_np.py) and a committed fixture, the KITTI flow file
format, the frame listing, the train command's flags, and the argument checks of of_flow_eval /
of_flow_upsample, which precede any launch.  No GPU work."""
import ctypes as C
import os

import numpy as np
import pytest

import kitti_flow_np as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY_PATH = os.path.join(ROOT, "tests", "golden", "kitti_flow_tiny.png")

# the samples tests/golden/make_kitti_flow_golden.py wrote, (R, G, B) per pixel
TINY = np.array([
    [(0, 0, 1), (32768, 32768, 1), (65535, 65535, 1), (32832, 32640, 1)],
    [(12345, 54321, 0), (0, 0, 0), (40000, 30000, 1), (32769, 32767, 1)],
    [(256, 1, 1), (1, 256, 1), (65535, 0, 1), (0x1234, 0x5678, 0x9ABC)],
], np.uint16)


@pytest.fixture(scope="module")
def lib():
    from optical_flow_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def _read_status(lib, path, shape=(64, 64, 3)):
    out = np.zeros(shape, np.uint16)
    h, w = C.c_int(), C.c_int()
    st = lib.of_png_read_u16(os.fsencode(path), out.ctypes.data_as(C.c_void_p), out.size,
                             C.byref(h), C.byref(w))
    return st, lib.of_last_error().decode(errors="replace"), out, (h.value, w.value)


def _random_u16(h, w, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 65536, (h, w, 3)).astype(np.uint16)
    img[0, 0] = (0, 32768, 65535)
    return img


# ---- decode -----------------------------------------------------------------------------------
def test_fixture_decodes_to_its_known_samples(lib):
    from optical_flow_amd.evaluate import read_flow_kitti, read_png_u16
    assert os.path.getsize(TINY_PATH) < 1024
    rgb = read_png_u16(TINY_PATH)
    assert rgb.dtype == np.uint16 and rgb.shape == (3, 4, 3)
    np.testing.assert_array_equal(rgb, TINY)                 # exact, R, G, B order, not reduced
    flow, valid = read_flow_kitti(TINY_PATH)
    assert flow.dtype == np.float32 and flow.shape == (3, 4, 2) and valid.dtype == np.bool_
    # R is x, G is y, B is valid
    np.testing.assert_array_equal(flow[0, 0], [-512.0, -512.0])
    np.testing.assert_array_equal(flow[0, 1], [0.0, 0.0])               # valid, zero flow
    np.testing.assert_array_equal(flow[0, 2], [65535 / 64 - 512, 65535 / 64 - 512])
    np.testing.assert_array_equal(flow[0, 3], [1.0, -2.0])
    np.testing.assert_array_equal(flow[1, 3], [1 / 64, -1 / 64])
    np.testing.assert_array_equal(flow[2, 0], [256 / 64 - 512, 1 / 64 - 512])
    np.testing.assert_array_equal(flow[2, 2], [65535 / 64 - 512, -512.0])
    np.testing.assert_array_equal(valid, [[1, 1, 1, 1], [0, 0, 1, 1], [1, 1, 1, 1]])
    np.testing.assert_array_equal(flow, (TINY[:, :, :2].astype(np.float64) - 32768) / 64)


@pytest.mark.parametrize("filt", [0, 1, 2, 3, 4, "cycle"])
@pytest.mark.parametrize("interlace", [False, True], ids=["plain", "adam7"])
def test_decodes_independent_files_of_every_filter(lib, tmp_path, filt, interlace):
    from optical_flow_amd.evaluate import read_png_u16
    for k, (h, w) in enumerate([(7, 11), (1, 1), (9, 8)]):
        img = _random_u16(h, w, 10 + k)
        path = str(tmp_path / ("f%d.png" % k))
        K.write_png(path, img, filt=filt, interlace=interlace)
        np.testing.assert_array_equal(read_png_u16(path), img)


@pytest.mark.parametrize("filt", [0, 1, 2, 3, 4, 5, 6])
def test_encoder_read_back_by_the_independent_reader(lib, tmp_path, filt):
    from optical_flow_amd.evaluate import read_png_u16, write_png_u16
    img = _random_u16(6, 13, 20 + filt)
    img[2:4] = img[1]                  # equal rows and smooth runs: the adaptive choice varies
    img[5] = np.arange(13 * 3).reshape(13, 3) * 100
    path = str(tmp_path / "w.png")
    write_png_u16(path, img, filt=filt)
    back, filters = K.read_png(path)
    assert back.dtype == np.uint16
    np.testing.assert_array_equal(back, img)
    if filt < 5:
        assert set(filters) == {filt}
    if filt == 6:
        assert filters == [y % 5 for y in range(6)]
    np.testing.assert_array_equal(read_png_u16(path), img)


def test_eight_bit_codec_is_unchanged(lib, tmp_path):
    """of_png_read_bgr still reduces a 16-bit file to its high bytes and of_png_write still
    writes 8-bit RGB, read back by the independent reader."""
    from optical_flow_amd.data_reader import imread_bgr, imwrite
    img16 = _random_u16(5, 9, 3)
    p16 = str(tmp_path / "a.png")
    K.write_png(p16, img16)
    np.testing.assert_array_equal(imread_bgr(p16), (img16 >> 8).astype(np.uint8)[:, :, ::-1])
    bgr = np.random.default_rng(4).integers(0, 256, (5, 9, 3)).astype(np.uint8)
    p8 = str(tmp_path / "b.png")
    imwrite(p8, bgr)
    back, _ = K.read_png(p8)
    assert back.dtype == np.uint8
    np.testing.assert_array_equal(back, bgr[:, :, ::-1])


def test_wrong_kind_of_png_is_refused(lib, tmp_path):
    from optical_flow_amd._lib import OF_EINVAL
    rgb8 = np.random.default_rng(0).integers(0, 256, (4, 5, 3)).astype(np.uint8)
    p = str(tmp_path / "rgb8.png")
    K.write_png(p, rgb8)
    st, msg, out, _ = _read_status(lib, p)
    assert st == OF_EINVAL and "bit depth 8" in msg and "colour type 2" in msg, msg
    assert not out.any()
    for depth, dt in ((8, np.uint8), (16, np.uint16)):
        p = str(tmp_path / ("gray%d.png" % depth))
        with open(p, "wb") as f:
            f.write(K.png_bytes(np.full((4, 5), 7, dt), ctype=0))
        st, msg, out, _ = _read_status(lib, p)
        assert st == OF_EINVAL and "colour type 0" in msg and "bit depth %d" % depth in msg, msg
        assert not out.any()


def test_truncated_file_is_refused(lib, tmp_path):
    from optical_flow_amd._lib import OF_EINVAL, OF_OK
    data = K.png_bytes(_random_u16(12, 17, 1))
    for cut in (len(data) - 1, len(data) - 12, len(data) // 2, 40, 20, 0):
        p = str(tmp_path / ("cut%d.png" % cut))
        with open(p, "wb") as f:
            f.write(data[:cut])
        st, msg, _, _ = _read_status(lib, p)
        assert st == OF_EINVAL and msg, (cut, msg)
    p = str(tmp_path / "whole.png")
    with open(p, "wb") as f:
        f.write(data)
    assert _read_status(lib, p)[0] == OF_OK
    # a buffer too small for the image, a missing file, NULL arguments
    out = np.zeros(10, np.uint16)
    h, w = C.c_int(), C.c_int()
    assert lib.of_png_read_u16(os.fsencode(p), out.ctypes.data_as(C.c_void_p), out.size,
                               C.byref(h), C.byref(w)) == OF_EINVAL
    assert b"too small" in lib.of_last_error()
    assert _read_status(lib, str(tmp_path / "none.png"))[0] == OF_EINVAL
    assert lib.of_png_read_u16(None, None, 0, None, None) == OF_EINVAL
    assert lib.of_png_write_u16(None, None, 1, 1, 0) == OF_EINVAL
    assert lib.of_png_write_u16(os.fsencode(str(tmp_path / "z.png")),
                                out.ctypes.data_as(C.c_void_p), 0, 3, 0) == OF_EINVAL


# ---- the KITTI flow format --------------------------------------------------------------------
def test_flow_round_trip_is_exact_and_clamps(lib, tmp_path):
    from optical_flow_amd.evaluate import read_flow_kitti, read_png_u16, write_flow_kitti
    rng = np.random.default_rng(2)
    flow = rng.integers(-32768, 32768, (9, 14, 2)).astype(np.float64) / 64.0   # multiples of 1/64
    flow[0, 0] = (-512.0, 511.984375)                                          # the range's ends
    valid = rng.uniform(size=(9, 14)) < 0.5
    p = str(tmp_path / "f.png")
    write_flow_kitti(p, flow, valid)
    back, v = read_flow_kitti(p)
    np.testing.assert_array_equal(back, flow.astype(np.float32))
    np.testing.assert_array_equal(v, valid)
    np.testing.assert_array_equal(read_png_u16(p)[:, :, 2], valid.astype(np.uint16))
    write_flow_kitti(p, flow)                                  # valid=None: valid everywhere
    assert read_flow_kitti(p)[1].all()
    # values outside the format clamp to its ends; others round to the nearest 1/64
    odd = np.array([[(-600.0, 600.0), (1e9, -1e9), (0.004, -0.012)]])
    write_flow_kitti(p, odd)
    np.testing.assert_array_equal(read_png_u16(p)[0, :, :2],
                                  [(0, 65535), (65535, 0), (32768, 32767)])


# ---- the frame listing ------------------------------------------------------------------------
def _touch(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "wb").close()


def test_list_kitti_flow(tmp_path):
    from optical_flow_amd.evaluate import list_kitti_flow
    tr = tmp_path / "data" / "training"
    for n in ("000010", "000002", "000007"):                 # complete frames, made out of order
        for rel in ("image_2/%s_10.png", "image_2/%s_11.png", "flow_occ/%s_10.png"):
            _touch(str(tr / (rel % n)))
    _touch(str(tr / "flow_noc" / "000007_10.png"))           # the only noc frame
    _touch(str(tr / "flow_occ" / "000003_10.png"))           # no images
    _touch(str(tr / "image_2" / "000004_10.png"))            # no second image
    _touch(str(tr / "flow_occ" / "000004_10.png"))
    _touch(str(tr / "image_2" / "000005_10.png"))            # no ground truth
    _touch(str(tr / "image_2" / "000005_11.png"))
    _touch(str(tr / "flow_occ" / "notes.txt"))
    for root in (tmp_path / "data", tr):                     # both root forms
        frames = list_kitti_flow(str(root))
        assert [os.path.basename(f[2]) for f in frames] == ["000002_10.png", "000007_10.png",
                                                            "000010_10.png"]
        for a, b, g in frames:
            n = os.path.basename(g)[:6]
            assert a == str(tr / "image_2" / (n + "_10.png"))
            assert b == str(tr / "image_2" / (n + "_11.png"))
            assert g == str(tr / "flow_occ" / (n + "_10.png"))
        noc = list_kitti_flow(root, gt="noc")                # a path object too
        assert [f[2] for f in noc] == [str(tr / "flow_noc" / "000007_10.png")]
    with pytest.raises(ValueError):
        list_kitti_flow(str(tr), gt="all")
    empty = tmp_path / "empty"
    os.makedirs(str(empty / "training" / "image_2"))
    with pytest.raises(FileNotFoundError) as e:
        list_kitti_flow(str(empty))
    assert str(empty / "training") in str(e.value)
    with pytest.raises(FileNotFoundError) as e:
        list_kitti_flow(str(tmp_path / "nowhere"))
    assert str(tmp_path / "nowhere") in str(e.value)


def test_bad_arguments_raise_value_error(lib):
    """Argument checks are exceptions, not asserts (they must survive python -O)."""
    import types
    from optical_flow_amd import evaluate as E
    net = types.SimpleNamespace(warp_convention="image")
    with pytest.raises(ValueError, match="no frames"):
        E.evaluate(net, [])
    with pytest.raises(ValueError, match="batch_size"):
        E.evaluate(net, [("a", "b", "c")], batch_size=0)
    with pytest.raises(ValueError, match="image"):
        E.evaluate(types.SimpleNamespace(), [("a", "b", "c")])
    a = np.zeros((4, 5, 3), np.uint8)
    with pytest.raises(ValueError, match="shape"):
        E.predict_flow(net, a, np.zeros((4, 6, 3), np.uint8))
    with pytest.raises(ValueError):
        E.pack_gt_raw([np.zeros((4, 5, 3), np.uint8)])
    with pytest.raises(ValueError):
        E.pack_gt_raw([np.zeros((4, 5), np.uint16)])
    with pytest.raises(ValueError):
        E.encode_flow_kitti(np.zeros((4, 5, 3)))
    with pytest.raises(ValueError):
        E.write_png_u16("unused.png", np.zeros((4, 5), np.uint16))
    with pytest.raises(ValueError):
        E.flow_metrics(np.zeros((1, 2, 2, 2), np.float32), [])
    with pytest.raises(ValueError):
        E.upsample_flow(np.zeros((1, 2, 2, 2), np.float32), 4, 4)


# ---- the train command ------------------------------------------------------------------------
def test_train_eval_flags():
    from optical_flow_amd.train import build_parser, check_eval_args, header_record
    ap = build_parser()
    args = ap.parse_args([])
    assert args.eval_kitti_flow is None and args.eval_every == 1
    check_eval_args(args)                                    # nothing asked: nothing to refuse
    assert header_record(args) is None
    with pytest.raises(ValueError):
        check_eval_args(ap.parse_args(["--eval-kitti-flow", "/data/kitti"]))
    with pytest.raises(ValueError):
        check_eval_args(ap.parse_args(["--eval-kitti-flow", "/data/kitti", "--warp-convention",
                                       "reference"]))
    with pytest.raises(ValueError):
        check_eval_args(ap.parse_args(["--eval-kitti-flow", "/data/kitti", "--warp-convention",
                                       "image", "--eval-every", "0"]))
    good = ap.parse_args(["--eval-kitti-flow", "/data/kitti", "--warp-convention", "image",
                          "--eval-every", "3"])
    check_eval_args(good)
    head = header_record(good)
    assert head["eval_kitti_flow"] == "/data/kitti" and head["eval_every"] == 3
    assert head["warp_convention"] == "image"
    assert "eval_kitti_flow" not in header_record(ap.parse_args(["--warp-convention", "image"]))


def test_train_refuses_eval_without_the_image_convention(capsys):
    """The parser errors (exit status 2, the flag named) before anything touches a device."""
    from optical_flow_amd.train import main
    with pytest.raises(SystemExit) as e:
        main(["--eval-kitti-flow", "/data/kitti", "--steps", "1"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--eval-kitti-flow" in err and "--warp-convention image" in err


# ---- argument checks of the kernels' entry points ---------------------------------------------
def test_flow_eval_argument_checks(lib):
    from optical_flow_amd._lib import OF_EINVAL, OF_OK
    from optical_flow_amd.evaluate import DESC_DTYPE
    # 64-byte aligned host memory stands in for the device pointers: every case is refused (or,
    # with n == 0, accepted) before anything is launched
    buf = np.zeros(4096 + 64, np.uint8)
    base = (buf.ctypes.data + 63) // 64 * 64
    flow, gt, part, out = (C.c_void_p(base + 1024 * k) for k in range(4))
    npart = lib.of_flow_eval_partials(2, 375, 1242)
    assert npart == 2 * 114 and lib.of_flow_eval_partials(1, 5, 7) == 1
    assert lib.of_flow_eval_partials(0, 5, 7) == 0 and lib.of_flow_eval_partials(-1, 5, 7) == 0
    assert lib.of_flow_eval_partials(3, 4000, 4000) == 3 * 256            # saturates
    desc = np.zeros(2, DESC_DTYPE)
    desc[0] = (256, 5, 7)
    desc[1] = (512, 3, 4)
    dp = desc.ctypes.data_as(C.c_void_p)

    def run(flow=flow, n=2, fh=4, fw=6, gt=gt, descs=dp, gt_bytes=1024, part=part, npart=2,
            out=out):
        return lib.of_flow_eval(flow, n, fh, fw, gt, descs, gt_bytes, part, npart, out, None)

    for bad in (dict(flow=None), dict(gt=None), dict(part=None), dict(out=None), dict(n=-1),
                dict(fh=0), dict(fw=0), dict(fh=-3), dict(npart=3), dict(npart=0),
                dict(npart=2 * 257), dict(n=70000, npart=70000)):
        assert run(**bad) == OF_EINVAL, bad
        assert b"flow eval" in lib.of_last_error()
    for k, field, value in ((0, "h", 0), (1, "w", 0), (1, "h", -2), (0, "offset", -256),
                            (0, "offset", 0), (1, "offset", 1024)):
        d = desc.copy()
        d[field][k] = value
        assert run(descs=d.ctypes.data_as(C.c_void_p)) == OF_EINVAL, (k, field, value)
        assert b"descriptor %d" % k in lib.of_last_error()
    assert run(n=0, npart=0) == OF_OK                                    # an empty batch
    assert run(n=0, npart=2) == OF_EINVAL


def test_flow_upsample_argument_checks(lib):
    from optical_flow_amd._lib import OF_EINVAL, OF_OK
    buf = np.zeros(1024, np.uint8)
    base = (buf.ctypes.data + 63) // 64 * 64
    flow, out = C.c_void_p(base), C.c_void_p(base + 512)

    def run(flow=flow, n=1, fh=2, fw=2, gh=4, gw=4, out=out):
        return lib.of_flow_upsample(flow, n, fh, fw, gh, gw, out, None)

    for bad in (dict(flow=None), dict(out=None), dict(n=-1), dict(fh=0), dict(fw=0), dict(gh=0),
                dict(gw=0), dict(gw=-5)):
        assert run(**bad) == OF_EINVAL, bad
        assert b"flow upsample" in lib.of_last_error()
    assert run(n=0) == OF_OK


# ---- the restatement and the inputs, on their own ground --------------------------------------
def test_restatement_basics():
    # a constant flow upsamples to the scaled constant, at any size
    f = np.broadcast_to(np.array([1.5, -2.25], np.float32), (3, 5, 2))
    np.testing.assert_allclose(K.upsample_np(f, 12, 10), np.broadcast_to([3.0, -9.0], (12, 10, 2)),
                               rtol=0, atol=1e-12)
    # equal sizes: the identity
    g = np.random.default_rng(0).standard_normal((4, 6, 2)).astype(np.float32)
    np.testing.assert_allclose(K.upsample_np(g, 4, 6), g, rtol=0, atol=1e-12)
    # x2: pixel 1 lies a quarter of the way from source 0 to source 1, border pixels replicate
    r = np.zeros((1, 2, 2), np.float32)
    r[0, 1] = (4.0, 8.0)
    np.testing.assert_allclose(K.upsample_np(r, 1, 4)[0, :, 0], [0.0, 2.0, 6.0, 8.0], atol=1e-12)
    # the outlier rule: 3 px and 5 %, a zero ground truth with epe > 3 is an outlier
    rgb = np.zeros((1, 4, 3), np.uint16)
    rgb[0, :, :2] = 32768
    rgb[0, :, 2] = (1, 1, 1, 0)
    rgb[0, 1, 0] = 32768 + 64 * 100                      # ground truth (100, 0)
    uv = np.array([[(3.5, 0.0), (104.0, 0.0), (2.5, 0.0), (50.0, 0.0)]])
    epe, mag, valid, outlier = K.epe_np(uv, rgb)
    np.testing.assert_allclose(epe[0], [3.5, 4.0, 2.5, 50.0])
    assert outlier[0].tolist() == [True, False, False, False] and valid[0].tolist()[3] is False


def test_inputs_keep_their_margins():
    flow, maps = K.make_case(8, 16, [(37, 61), (33, 67), (13, 21)], 1)
    m3, m5 = K.margins_np(flow, maps)
    assert m3 >= 0.1 and m5 >= 1e-3, (m3, m5)
    s, v, o = K.flow_eval_np(flow, maps)
    assert (v > 0).all() and (o > 0).all() and (o < v).all()
    # every branch: below 3 px, outliers, above 3 px but within 5 %
    saved = 0
    for f, rgb in zip(flow, maps):
        epe, mag, valid, outlier = K.epe_np(K.upsample_np(f, *rgb.shape[:2]), rgb)
        saved += int((valid & (epe > 3.0) & ~outlier).sum())
    assert saved > 0
