"""Host side of the training augmentation: the seeded parameter draw (sample_augment), the
option checks, the of_augment record layout and the train command's flags.  No GPU work."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _opts(**kw):
    from optical_flow_amd.data_reader import AugmentOpts
    return AugmentOpts(**kw)


FULL = dict(zoom=(1.0, 2.0), hflip_prob=0.5, rotate_deg=10.0, brightness=0.1,
            contrast=(0.8, 1.2), saturation=(0.7, 1.3), color_gain=(0.9, 1.1))


def test_sample_is_deterministic_in_seed_and_batch_index():
    from optical_flow_amd.data_reader import sample_augment
    o = _opts(**FULL)
    a = sample_augment(o, 4, 48, 64, 3, 5)
    assert a.shape == (4,)
    assert a.tobytes() == sample_augment(o, 4, 48, 64, 3, 5).tobytes()
    assert a.tobytes() != sample_augment(o, 4, 48, 64, 4, 5).tobytes()      # another seed
    assert a.tobytes() != sample_augment(o, 4, 48, 64, 3, 6).tobytes()      # another batch
    assert a.tobytes() != sample_augment(o, 4, 48, 64, 5, 3).tobytes()      # not symmetric
    assert len({r.tobytes() for r in a}) == 4                               # a draw per pair


def test_default_is_the_plain_full_frame_map():
    from optical_flow_amd.data_reader import sample_augment
    for oh, ow in [(48, 64), (19, 23), (384, 512)]:
        rec = sample_augment(_opts(), 3, oh, ow, 0, 0)
        exp = np.array([1.0 / ow, 0, 0, 0, 1.0 / oh, 0]).astype(np.float32)
        for r in rec:
            np.testing.assert_array_equal(r["m"], exp)
            assert r["flags"] == 0
            np.testing.assert_array_equal(r["gain"], np.ones(3, np.float32))
            assert (r["brightness"], r["contrast"], r["saturation"]) == (0.0, 1.0, 1.0)
        assert not rec["pad"].any()


@pytest.mark.parametrize("translate", [True, False])
def test_crop_window_stays_inside_the_frame(translate):
    from optical_flow_amd.data_reader import sample_augment
    o = _opts(zoom=(1.0, 2.0), translate=translate, hflip_prob=0.5)
    oh, ow = 37, 61
    zooms = []
    for k in range(50):                                      # 50 batches of 4: 200 draws
        for r in sample_augment(o, 4, oh, ow, 11, k):
            m = r["m"].astype(np.float64)
            for xc in (0.0, ow):
                for yc in (0.0, oh):
                    u = m[0] * xc + m[1] * yc + m[2]
                    v = m[3] * xc + m[4] * yc + m[5]
                    assert -1e-6 <= u <= 1 + 1e-6 and -1e-6 <= v <= 1 + 1e-6, (k, m)
            assert m[1] == 0 and m[3] == 0
            zooms.append(1.0 / (abs(m[0]) * ow))
            np.testing.assert_allclose(1.0 / (m[4] * oh), zooms[-1], rtol=1e-6)
            if not translate:                                # centred window
                assert abs(m[0] * ow / 2 + m[2] - 0.5) < 1e-6
                assert abs(m[4] * oh / 2 + m[5] - 0.5) < 1e-6
    assert 1 - 1e-6 <= min(zooms) and max(zooms) <= 2 + 1e-6 and max(zooms) - min(zooms) > 0.5


def test_hflip_sign():
    from optical_flow_amd.data_reader import sample_augment
    assert (sample_augment(_opts(hflip_prob=1.0), 16, 20, 30, 1, 0)["m"][:, 0] < 0).all()
    assert (sample_augment(_opts(hflip_prob=0.0), 16, 20, 30, 1, 0)["m"][:, 0] > 0).all()
    both = sample_augment(_opts(hflip_prob=0.5), 64, 20, 30, 1, 0)["m"][:, 0]
    assert (both < 0).any() and (both > 0).any()
    # a flipped full frame maps the left edge to u = 1
    m = sample_augment(_opts(hflip_prob=1.0), 1, 20, 30, 1, 0)["m"][0].astype(np.float64)
    assert abs(m[2] - 1.0) < 1e-6 and abs(m[0] * 30 + m[2]) < 1e-6


def test_rotation_is_about_the_output_centre():
    from optical_flow_amd.data_reader import sample_augment
    oh, ow = 40, 70
    rec = sample_augment(_opts(rotate_deg=20.0), 32, oh, ow, 2, 0)
    angles = []
    for r in rec:
        m = r["m"].astype(np.float64)
        # the output centre maps to the frame centre whatever the angle
        assert abs(m[0] * ow / 2 + m[1] * oh / 2 + m[2] - 0.5) < 1e-6
        assert abs(m[3] * ow / 2 + m[4] * oh / 2 + m[5] - 0.5) < 1e-6
        # in output-pixel units the linear part is a rotation
        lin = np.array([[m[0] * ow, m[1] * ow], [m[3] * oh, m[4] * oh]])
        np.testing.assert_allclose(lin @ lin.T, np.eye(2), atol=1e-5)
        angles.append(np.degrees(np.arctan2(lin[1, 0], lin[0, 0])))
    assert max(np.abs(angles)) <= 20.0 + 1e-4 and min(angles) < -2 and max(angles) > 2


def test_colour_parameters_lie_in_their_ranges():
    from optical_flow_amd.data_reader import sample_augment
    o = _opts(**FULL)
    recs = np.concatenate([sample_augment(o, 8, 32, 48, 9, k) for k in range(25)])
    f32 = np.float32
    assert (recs["flags"] == 1).all()
    assert (np.abs(recs["brightness"]) <= f32(0.1)).all() and np.ptp(recs["brightness"]) > 0.1
    for name, (lo, hi) in (("contrast", (0.8, 1.2)), ("saturation", (0.7, 1.3)),
                           ("gain", (0.9, 1.1))):
        v = recs[name]
        assert (v >= f32(lo)).all() and (v <= f32(hi)).all(), name
        assert np.ptp(v) > 0.5 * (hi - lo), name
    g = recs["gain"]
    assert (g[:, 0] != g[:, 1]).any() and (g[:, 1] != g[:, 2]).any()   # drawn per channel


@pytest.mark.parametrize("kw,flag", [(dict(), 0), (dict(zoom=(1.0, 1.5), hflip_prob=0.5), 0),
                                     (dict(brightness=0.1), 1), (dict(contrast=(0.9, 1.0)), 1),
                                     (dict(saturation=(1.0, 1.1)), 1),
                                     (dict(color_gain=(0.9, 1.1)), 1)])
def test_flags_bit0_only_with_a_colour_range(kw, flag):
    from optical_flow_amd.data_reader import sample_augment
    assert (sample_augment(_opts(**kw), 4, 16, 16, 0, 0)["flags"] == flag).all()


def test_geometry_draws_do_not_depend_on_the_colour_options():
    """Every draw is made for every batch in a fixed order, so switching one option on leaves
    the other parameters of the same (seed, batch_index) as they were."""
    from optical_flow_amd.data_reader import sample_augment
    geo = dict(zoom=(1.0, 1.5), hflip_prob=0.5, rotate_deg=5.0)
    a = sample_augment(_opts(**geo), 4, 32, 48, 7, 3)
    b = sample_augment(_opts(brightness=0.2, color_gain=(0.8, 1.2), **geo), 4, 32, 48, 7, 3)
    np.testing.assert_array_equal(a["m"], b["m"])


BAD = [dict(zoom=(1.5, 1.2)), dict(zoom=(0.9, 1.2)), dict(contrast=(1.2, 0.8)),
       dict(saturation=(1.1, 1.0)), dict(color_gain=(1.2, 1.1)), dict(hflip_prob=-0.1),
       dict(hflip_prob=1.5), dict(hflip_prob=float("nan")), dict(zoom=(1.0, float("inf"))),
       dict(brightness=float("nan")), dict(rotate_deg=float("inf")),
       dict(contrast=(float("nan"), 1.0)), dict(saturation=(1.0, float("inf"))),
       dict(color_gain=(float("-inf"), 1.0)), dict(brightness=-0.1), dict(rotate_deg=-5.0)]


@pytest.mark.parametrize("kw", BAD, ids=[repr(b) for b in BAD])
def test_bad_options_raise(kw):
    with pytest.raises(ValueError):
        _opts(**kw)


def test_reader_opts_default_has_no_augmentation():
    from optical_flow_amd.data_reader import ReaderOpts
    assert ReaderOpts("/nowhere", 4, 16, 24, 2).augment is None
    # the new keyword is the last one: the positional form of every older argument still binds
    o = ReaderOpts("/nowhere", 4, 16, 24, 2, 5, 3, None, 10, 12)
    assert (o.seed, o.nslots, o.pairs, o.max_h, o.max_w, o.augment) == (5, 3, None, 10, 12, None)
    a = _opts(hflip_prob=0.5)
    assert ReaderOpts("/nowhere", 4, 16, 24, 2, augment=a).augment is a


def test_record_layout_matches_the_c_struct():
    from optical_flow_amd.data_reader import AUGMENT_DTYPE
    import augment_np
    assert AUGMENT_DTYPE.itemsize == 64
    # typedef struct of_augment { float m[6]; float gain[3]; float brightness, contrast,
    # saturation; int32_t flags; int32_t pad[3]; }
    exp = {"m": (0, np.float32, (6,)), "gain": (24, np.float32, (3,)),
           "brightness": (36, np.float32, ()), "contrast": (40, np.float32, ()),
           "saturation": (44, np.float32, ()), "flags": (48, np.int32, ()),
           "pad": (52, np.int32, (3,))}
    assert set(AUGMENT_DTYPE.names) == set(exp)
    for name, (off, base, shape) in exp.items():
        dt, o = AUGMENT_DTYPE.fields[name][:2]
        assert o == off and dt.base == np.dtype(base) and dt.shape == shape, name
    assert augment_np.AUGMENT_DTYPE == AUGMENT_DTYPE
    # and the header declares the same members in the same order
    src = open(os.path.join(ROOT, "include", "oflow.h")).read()
    body = src[src.index("typedef struct of_augment {"):src.index("} of_augment;")]
    order = [body.index(s) for s in ("float m[6]", "float gain[3]", "float brightness",
                                     "float contrast", "float saturation", "int32_t flags",
                                     "int32_t pad[3]")]
    assert order == sorted(order)


def test_restatement_identity_is_a_copy():
    """augment_np on its own ground: the identity record at equal power-of-two sizes returns the
    frame, normalised as oracle.data_np.normalise does."""
    import augment_np
    from oracle import data_np as D
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (32, 64, 3)).astype(np.uint8)
    rec = np.array([augment_np.identity(32, 64)])
    out = augment_np.augment_pairs([(img, img)], 32, 64, rec)
    np.testing.assert_array_equal(out[0, :, :, :3], D.normalise(img))
    np.testing.assert_array_equal(out[0, :, :, 3:], D.normalise(img))


def test_train_help_lists_the_augment_flags():
    r = subprocess.run([sys.executable, "-m", "optical_flow_amd.train", "--help"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ("--augment", "--aug-zoom-max", "--aug-hflip", "--aug-rotate", "--aug-brightness",
                 "--aug-contrast", "--aug-saturation", "--aug-color-gain"):
        assert flag in r.stdout, flag


@pytest.mark.parametrize("flags", [["--augment"], ["--aug-hflip", "0.5"]])
def test_augment_without_kitti_is_refused(flags):
    r = subprocess.run([sys.executable, "-m", "optical_flow_amd.train", "--steps", "1"] + flags,
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "--kitti" in r.stderr


def test_preset_and_overrides():
    from optical_flow_amd.train import augment_from_args, build_parser
    ap = build_parser()
    assert augment_from_args(ap.parse_args([])) is None
    p = augment_from_args(ap.parse_args(["--augment"]))
    assert p.as_dict() == {"zoom": [1.0, 1.3], "translate": True, "hflip_prob": 0.5,
                           "rotate_deg": 0.0, "brightness": 0.1, "contrast": [0.8, 1.2],
                           "saturation": [0.8, 1.2], "color_gain": [0.9, 1.1]}
    q = augment_from_args(ap.parse_args(["--augment", "--aug-zoom-max", "1.5", "--aug-hflip", "0",
                                         "--aug-rotate", "3", "--aug-contrast", "0.1"]))
    assert q.zoom == (1.0, 1.5) and q.hflip_prob == 0.0 and q.rotate_deg == 3.0
    assert q.contrast == (0.9, 1.1) and q.saturation == (0.8, 1.2)
    # an override alone switches augmentation on with every other field at its identity
    o = augment_from_args(ap.parse_args(["--aug-brightness", "0.2"]))
    assert o.brightness == 0.2 and o.zoom == (1.0, 1.0) and o.hflip_prob == 0.0
    with pytest.raises(ValueError):
        augment_from_args(ap.parse_args(["--aug-zoom-max", "0.5"]))
