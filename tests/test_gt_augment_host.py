"""Labelled augmentation without a GPU: the fp32 restatement of of_gt_augment against an
independent float64 one, its known answers (identity, flip, degenerate records, the 16-bit
range), the C entry's argument checks, the labelled reader's seeded records and the train
command's flags."""
import ctypes as C
import os

import numpy as np
import pytest

import gt_augment_ref as G
import kitti_flow_np as K

LSB = 1.0 / 64.0
NEAR = 1e-3          # source coordinates this close to an integer decide nothing in fp32


# ------------------------------------------------------------------ the reference ----
@pytest.mark.parametrize("name", ["identity", "flip", "zoom", "rotate", "preset1", "preset2"])
def test_float32_restatement_against_float64(name):
    recs = G.record_sets()[name]
    excluded = total = 0
    for i, rgb in enumerate(G.maps()):
        out = G.gt_augment_f32(rgb, recs[i], G.IMG_HW)
        got_valid, got = G.decode(out)
        valid, vec, su, sv = G.gt_augment_f64(rgb, recs[i], G.IMG_HW)
        near = (np.abs(su - np.rint(su)) < NEAR) | (np.abs(sv - np.rint(sv)) < NEAR)
        excluded += int(near.sum())
        total += near.size
        keep = ~near
        assert np.array_equal(got_valid[keep], valid[keep])
        both = keep & valid
        assert both.any()
        err = np.abs(got[both] - vec[both]).max()
        print("%s map %d: %d valid, max |fp32 - float64| = %.4f px" % (name, i, both.sum(), err))
        assert err <= LSB
        assert not out[~got_valid].any() and (out[got_valid][:, 2] == 1).all()
    print("%s: %d of %d pixels within %g of a pixel edge" % (name, excluded, total, NEAR))
    assert excluded <= 0.01 * total


def test_identity_record_keeps_the_valid_pixels():
    for rgb in G.maps():
        for H, W in (G.IMG_HW, (64, 128), (375, 1242)):
            out = G.gt_augment_f32(rgb, G.identity(H, W), (H, W))
            valid = rgb[..., 2] != 0
            assert np.array_equal(out[..., 2], valid.astype(np.uint16))     # B normalised to 1
            assert np.array_equal(out[valid][:, :2], rgb[valid][:, :2])
            assert not out[~valid].any()


def test_pure_flip_mirrors_the_map_and_negates_u():
    H, W = G.IMG_HW
    for rgb in G.maps():
        out = G.gt_augment_f32(rgb, G.flip(H, W), (H, W))
        src = rgb[:, ::-1]
        valid = src[..., 2] != 0
        assert np.array_equal(out[..., 2] != 0, valid)
        # -u on the 1/64 grid: 32768 - (R - 32768); R = 0 would need 65536 and is not in the maps
        assert np.array_equal(out[valid][:, 0].astype(np.int64), 65536 - src[valid][:, 0].astype(np.int64))
        assert np.array_equal(out[valid][:, 1], src[valid][:, 1])
        assert not out[~valid].any()


@pytest.mark.parametrize("m", [[0.0] * 6, [float("nan")] * 6,
                               [float("inf"), 0.0, 0.0, 0.0, 1.0 / 16, 0.0]])
def test_degenerate_records_give_an_invalid_map(m):
    rgb = G.maps()[0]
    assert not G.gt_augment_f32(rgb, G.record(m), G.IMG_HW).any()
    assert not G.gt_augment_f64(rgb, G.record(m), G.IMG_HW)[0].any()


def test_a_nan_translation_invalidates_without_a_degenerate_determinant():
    H, W = G.IMG_HW
    m = [1.0 / W, 0.0, float("nan"), 0.0, 1.0 / H, 0.0]
    assert not G.gt_augment_f32(G.maps()[0], G.record(m), G.IMG_HW).any()


def test_a_vector_that_leaves_the_16_bit_range_becomes_invalid():
    H, W = G.IMG_HW
    rgb = np.ones((6, 8, 3), np.uint16)
    rgb[..., 0] = 32768 + 64 * 300            # 300 px: 390 px under zoom 1.3, still in range
    rgb[..., 1] = 32768
    rgb[2, 3, 0] = 32768 + 64 * 400           # 400 px: 520 px, past the format's 511.98
    rgb[4, 5, 1] = 32768 - 64 * 400           # -520 px, below its -512
    rec = G.zoom(H, W, 1.3)
    out = G.gt_augment_f32(rgb, rec, (H, W))
    valid, vec, su, sv = G.gt_augment_f64(rgb, rec, (H, W))
    xs, ys = np.floor(su).astype(int), np.floor(sv).astype(int)
    hit = ((xs == 3) & (ys == 2)) | ((xs == 5) & (ys == 4))
    assert hit.any() and not hit.all()
    assert np.array_equal(out[..., 2] != 0, ~hit) and np.array_equal(valid, ~hit)
    assert not out[hit].any()                                   # not clamped to 65535 or 0
    assert (out[~hit][:, 0] == 32768 + 64 * 390).all()


# ------------------------------------------------------------ the C entry's checks ----
@pytest.fixture(scope="module")
def lib():
    from optical_flow_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


DESC = np.dtype([("offset", np.int64), ("h", np.int32), ("w", np.int32)])


def _descs(*rows):
    d = np.zeros(len(rows), DESC)
    for i, r in enumerate(rows):
        d[i] = r
    return d


def _call(lib, **over):
    """of_gt_augment with every argument valid except ``over``; the pointers are host buffers,
    which no call here ever reaches a launch with."""
    buf = (C.c_float * 1024)()
    base = C.addressof(buf)
    base += (-base) % 16
    a = dict(raw=base, descs=_descs((256, 4, 5), (512, 3, 3)), gt_bytes=1024, n=2, img_h=16,
             img_w=32, params=base + 2048, out=base + 1024, _keep=buf)
    a.update(over)
    d = a["descs"]
    return lib.of_gt_augment(a["raw"], d.ctypes.data_as(C.c_void_p) if d is not None else None,
                             a["gt_bytes"], a["n"], a["img_h"], a["img_w"], a["params"], a["out"],
                             None)


def _aligned(extra=0):
    buf = (C.c_float * 1024)()
    base = C.addressof(buf)
    return buf, base + (-base) % 16 + extra


BAD = [("raw", dict(raw=None)), ("descs", dict(descs=None)), ("params", dict(params=None)),
       ("out", dict(out=None)), ("n-1", dict(n=-1)), ("n65536", dict(n=65536)),
       ("img_h0", dict(img_h=0)), ("img_w0", dict(img_w=0)),
       ("gt_bytes0", dict(gt_bytes=0)),
       ("desc size", dict(descs=_descs((256, 0, 5), (512, 3, 3)))),
       ("desc in header", dict(descs=_descs((0, 4, 5), (512, 3, 3)))),
       ("desc past end", dict(descs=_descs((256, 4, 5), (1020, 3, 3))))]


@pytest.mark.parametrize("name,over", BAD, ids=[b[0] for b in BAD])
def test_einval(lib, name, over):
    assert _call(lib, **over) == 1                     # OF_EINVAL, no exception, no launch
    assert b"gt augment" in lib.of_last_error()


def test_einval_for_aliased_and_misaligned_buffers(lib):
    keep, base = _aligned()
    assert _call(lib, raw=base, out=base) == 1 and b"must not be" in lib.of_last_error()
    assert _call(lib, raw=base + 8, out=base + 2048) == 1 and b"16-byte" in lib.of_last_error()
    assert _call(lib, raw=base, out=base + 2048 + 4) == 1 and b"16-byte" in lib.of_last_error()


def test_no_maps_is_ok_and_launches_nothing(lib):
    assert _call(lib, n=0) == 0 and _call(lib, n=0, gt_bytes=0) == 0


def test_ops_augment_gt_needs_a_gpu_and_matching_records():
    from optical_flow_amd import ops
    from optical_flow_amd.gt_raw import pack_gt_raw
    import torch
    raw, descs = pack_gt_raw(G.maps())
    with pytest.raises(ValueError, match="CUDA uint8"):        # no CPU fall-back
        ops.augment_gt((torch.from_numpy(raw), descs), G.record_sets()["flip"], G.IMG_HW)
    with pytest.raises(ValueError, match="host descriptors"):
        ops._gt_handle(torch.from_numpy(raw), 3)


# ------------------------------------------------------------------ labelled reader ----
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """Five tiny labelled frames of two native sizes in KITTI's layout."""
    root = str(tmp_path_factory.mktemp("kitti_flow_aug"))
    tr = os.path.join(root, "training")
    for d in ("image_2", "flow_occ"):
        os.makedirs(os.path.join(tr, d))
    rng = np.random.default_rng(7)
    for k in range(5):
        h, w = ((9, 14), (7, 12))[k % 2]
        for rel in ("image_2/%06d_10.png", "image_2/%06d_11.png"):
            K.write_png(os.path.join(tr, rel % k), rng.integers(0, 256, (h, w, 3)).astype(np.uint8))
        K.write_png(os.path.join(tr, "flow_occ/%06d_10.png" % k), G.make_map(h, w, rng))
    return root


def test_reader_records_are_seeded_and_differ_per_epoch(tree):
    from optical_flow_amd.data_reader import sample_augment
    from optical_flow_amd.evaluate import KittiFlowReader
    opts = G.preset_opts()
    r = KittiFlowReader(tree, 2, 16, 32, seed=3, nworkers=2, label_augment=opts)
    assert r.nbatches == 2
    for e in range(3):
        for k in range(2):
            want = sample_augment(opts, 2, 16, 32, 3, e * 2 + k)
            assert r.records(e, k).tobytes() == want.tobytes()
    again = KittiFlowReader(tree, 2, 16, 32, seed=3, label_augment=G.preset_opts())
    assert again.records(1, 1).tobytes() == r.records(1, 1).tobytes()
    seen = {r.records(e, k)["m"].tobytes() for e in range(3) for k in range(2)}
    assert len(seen) == 6                                          # every batch of every epoch
    other = KittiFlowReader(tree, 2, 16, 32, seed=4, label_augment=opts)
    assert other.records(0, 0).tobytes() != r.records(0, 0).tobytes()
    for bad in ((0, 2), (0, -1), (-1, 0)):
        with pytest.raises(ValueError):
            r.records(*bad)


def test_reader_without_label_augment_is_unchanged(tree):
    from optical_flow_amd.data_reader import AugmentOpts
    from optical_flow_amd.evaluate import KittiFlowReader
    plain = KittiFlowReader(tree, 2, 16, 32, seed=3, nworkers=2)
    none = KittiFlowReader(tree, 2, 16, 32, seed=3, nworkers=2, label_augment=None)
    aug = KittiFlowReader(tree, 2, 16, 32, seed=3, nworkers=2, label_augment=G.preset_opts())
    assert plain.label_augment is None and none.label_augment is None
    with pytest.raises(ValueError, match="label_augment"):
        plain.records(0, 0)
    ref = list(plain.host_batches(1))
    for other in (none, aug):                   # the host side never augments: same frames, maps
        assert other.order(1) == plain.order(1)
        for (p0, m0, i0), (p1, m1, i1) in zip(ref, other.host_batches(1)):
            assert i0 == i1
            assert all(np.array_equal(a, b) for x, y in zip(p0, p1) for a, b in zip(x, y))
            assert all(np.array_equal(a, b) for a, b in zip(m0, m1))
    with pytest.raises(ValueError, match="augment"):             # the old keyword still refuses
        KittiFlowReader(tree, 2, 16, 32, augment=AugmentOpts())
    with pytest.raises(TypeError, match="label_augment"):
        KittiFlowReader(tree, 2, 16, 32, label_augment={"zoom": (1.0, 1.3)})


# ------------------------------------------------------------------ train command ----
def _parse(argv):
    from optical_flow_amd.train import build_parser
    return build_parser().parse_args(argv)


BASE = ["--kitti-flow", "/x", "--warp-convention", "image"]


def test_flags_build_the_options():
    from optical_flow_amd.train import AUGMENT_PRESET, kitti_flow_augment_from_args
    assert kitti_flow_augment_from_args(_parse([])) is None
    assert kitti_flow_augment_from_args(_parse(BASE)) is None
    o = kitti_flow_augment_from_args(_parse(BASE + ["--kitti-flow-augment"]))
    assert o.as_dict() == G.preset_opts().as_dict()
    o = kitti_flow_augment_from_args(_parse(BASE + ["--kitti-flow-augment",
                                                    "--kitti-flow-aug-zoom-max", "1.5",
                                                    "--kitti-flow-aug-rotate", "3"]))
    assert o.zoom == (1.0, 1.5) and o.rotate_deg == 3.0
    assert o.hflip_prob == AUGMENT_PRESET["hflip_prob"] and o.has_color
    # each override works without the preset, from the identity
    o = kitti_flow_augment_from_args(_parse(BASE + ["--kitti-flow-aug-hflip", "0.25"]))
    assert o.hflip_prob == 0.25 and o.zoom == (1.0, 1.0) and not o.has_color
    o = kitti_flow_augment_from_args(_parse(BASE + ["--kitti-flow-aug-zoom-max", "1.2"]))
    assert o.zoom == (1.0, 1.2) and o.hflip_prob == 0.0
    o = kitti_flow_augment_from_args(_parse(BASE + ["--kitti-flow-aug-rotate", "5"]))
    assert o.rotate_deg == 5.0 and o.zoom == (1.0, 1.0)
    with pytest.raises(ValueError):
        kitti_flow_augment_from_args(_parse(BASE + ["--kitti-flow-aug-zoom-max", "0.5"]))


def test_header_record_gains_the_options_only_when_on():
    from optical_flow_amd.train import header_record, kitti_flow_augment_from_args
    a = _parse(BASE + ["--supervised-weight", "1", "--photometric-weight", "0"])
    off = header_record(a, None, kitti_flow_augment_from_args(a))
    assert off == header_record(a) and "kitti_flow_augment" not in off
    b = _parse(BASE + ["--supervised-weight", "1", "--photometric-weight", "0",
                       "--kitti-flow-augment"])
    opts = kitti_flow_augment_from_args(b)
    on = header_record(b, None, opts)
    assert on.pop("kitti_flow_augment") == opts.as_dict() and on == off
    assert "augment" not in on
    assert header_record(_parse([])) is None


@pytest.mark.parametrize("argv", [
    ["--kitti-flow-augment"],                                              # no --kitti-flow
    ["--kitti-flow-aug-hflip", "0.5", "--warp-convention", "image"],
    ["--kitti-flow-augment", "--kitti", "/y", "--warp-convention", "image"],
    ["--kitti-flow-augment", "--kitti-flow", "/x"],                        # reference convention
    ["--kitti-flow-aug-zoom-max", "1.3", "--kitti-flow", "/x"],
    ["--kitti-flow-aug-rotate", "5", "--kitti-flow", "/x"],
])
def test_train_command_rejects(argv, capsys):
    from optical_flow_amd.train import (check_kitti_flow_augment_args,
                                        kitti_flow_augment_from_args, main)
    a = _parse(argv)
    with pytest.raises(ValueError):
        check_kitti_flow_augment_args(a, kitti_flow_augment_from_args(a))
    with pytest.raises(SystemExit) as e:                # main: a parser error, before any GPU work
        main(argv)
    assert e.value.code == 2
    assert "--kitti-flow-augment" in capsys.readouterr().err


def test_bad_values_and_the_old_refusal_are_parser_errors(capsys):
    from optical_flow_amd.train import main
    for argv in (BASE + ["--kitti-flow-aug-hflip", "1.5"], BASE + ["--kitti-flow-aug-zoom-max", "0.9"],
                 BASE + ["--kitti-flow-augment", "--augment"]):       # --augment still refused
        with pytest.raises(SystemExit) as e:
            main(argv)
        assert e.value.code == 2
    capsys.readouterr()
