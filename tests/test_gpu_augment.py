"""GPU parity of the training augmentation: of_augment_pairs against its numpy float32
restatement (tests/augment_np.py) bit for bit, the identity record against of_preprocess_pairs,
the augmenting AsyncReader hand-out (of_reader_next_aug) across epoch wraps, the driver's
--augment run and the argument checks."""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

import augment_np as A
from oracle import data_np as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def lib():
    from optical_flow_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load()


# (first frame, second frame) -> output; every batch holds 3 pairs, so grid.y = 3
SIZES = [((37, 61), (38, 63), (19, 23)),    # 437 pixels: two workgroups, the second partial
         ((17, 29), (18, 31), (40, 70)),    # upscale
         ((2, 3), (3, 5), (5, 7)),
         ((1, 1), (1, 1), (3, 5)),          # every tap clamps
         ((64, 96), (65, 98), (32, 48))]


def _rotation(deg, oh, ow, z=1.0):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    a = [[c / z, -s / z], [s / z, c / z]]
    t = [a[0][0] * -ow / 2 + a[0][1] * -oh / 2 + ow / 2, a[1][0] * -ow / 2 + a[1][1] * -oh / 2 + oh / 2]
    return [a[0][0] / ow, a[0][1] / ow, t[0] / ow, a[1][0] / oh, a[1][1] / oh, t[1] / oh]


def _zoom2(oh, ow):
    return [0.5 / ow, 0.0, 0.3, 0.0, 0.5 / oh, 0.1]          # window (0.3, 0.1)-(0.8, 0.6)


# gain / brightness / contrast drive the [0, 1] clamp both ways on 8-bit noise:
# 1.0 -> ((1.6 - 0.15) - 0.5) * 1.7 + 0.5 > 1 and 0.0 -> (-0.15 - 0.5) * 1.7 + 0.5 < 0
COLOUR = dict(gain=(1.6, 0.5, 1.2), brightness=-0.15, contrast=1.7, saturation=1.4, flags=1)
COLOUR2 = dict(gain=(0.9, 1.1, 1.05), brightness=0.07, contrast=0.8, saturation=0.6, flags=1)


def _records(name, oh, ow):
    """Three of_augment records (one per pair) of the named parameter set."""
    same = {"identity": lambda: A.identity(oh, ow),
            "hflip": lambda: A.record([-1.0 / ow, 0.0, 1.0, 0.0, 1.0 / oh, 0.0]),
            "zoom2": lambda: A.record(_zoom2(oh, ow)),
            "rot20": lambda: A.record(_rotation(20.0, oh, ow)),
            "colour": lambda: A.record([0.8 / ow, 0.0, 0.15, 0.0, 0.8 / oh, 0.05], **COLOUR)}
    if name in same:
        return np.array([same[name]()] * 3)
    assert name == "mixed"
    return np.array([A.record(_rotation(-20.0, oh, ow, z=1.3), **COLOUR),
                     A.record([-1.0 / ow, 0.0, 1.0, 0.0, 1.0 / oh, 0.0]),
                     A.record(_zoom2(oh, ow), **COLOUR2)])


def _frames(rng, s1, s2):
    """Three pairs, ragged inside the batch: (s1, s2), (s2, s1), (s1, s1)."""
    img = lambda s: rng.integers(0, 256, s + (3,)).astype(np.uint8)
    return [(img(s1), img(s2)), (img(s2), img(s1)), (img(s1), img(s1))]


@pytest.mark.parametrize("params", ["identity", "hflip", "zoom2", "rot20", "colour", "mixed"])
@pytest.mark.parametrize("s1,s2,dst", SIZES, ids=["%dx%d-%dx%d" % (s[0] + s[2]) for s in SIZES])
def test_augment_pairs_bit_exact(s1, s2, dst, params):
    from optical_flow_amd.data_reader import augment_frames
    oh, ow = dst
    frames = _frames(np.random.default_rng(sum(s1) + oh), s1, s2)
    rec = _records(params, oh, ow)
    exp = A.augment_pairs(frames, oh, ow, rec)
    got = augment_frames(frames, oh, ow, rec).cpu().numpy()
    np.testing.assert_array_equal(got, exp)
    if params == "colour" and s1[0] > 2:
        # the case means what it says: both ends of the clamp occur in the expected output
        lo = (np.float64(np.float32(0)) - A.IMAGE_MEANS).astype(np.float32)
        hi = (np.float64(np.float32(1)) - A.IMAGE_MEANS).astype(np.float32)
        flat = exp.reshape(-1, 2, 3)
        assert (flat == lo).any() and (flat == hi).any()
    if params == "rot20" and s1[0] > 2:
        # samples leave the frame: the border is replicated there
        m = rec[0]["m"].astype(np.float64)
        assert m[2] < 0 or m[5] < 0 or m[0] * ow + m[2] > 1 or m[4] * oh + m[5] > 1


def test_identity_record_equals_preprocess_pairs():
    """Equal power-of-two sizes make the coordinate arithmetic exact and cv::resize a copy, so
    the identity record reproduces of_preprocess_pairs without going through augment_np."""
    from optical_flow_amd.data_reader import (AugmentOpts, augment_frames, preprocess_frames,
                                              sample_augment)
    rng = np.random.default_rng(5)
    img = lambda: rng.integers(0, 256, (32, 64, 3)).astype(np.uint8)
    frames = [(img(), img()) for _ in range(3)]
    rec = sample_augment(AugmentOpts(), 3, 32, 64, 0, 0)       # the default record, flags = 0
    assert (rec["flags"] == 0).all()
    got = augment_frames(frames, 32, 64, rec)
    exp = preprocess_frames(frames, 32, 64)
    assert torch.equal(got, exp)
    np.testing.assert_array_equal(got.cpu().numpy(), D.preprocess_pairs(frames, 32, 64))


@pytest.fixture(scope="module")
def kitti_tree(tmp_path_factory):
    from test_data_path import make_kitti
    root = tmp_path_factory.mktemp("kitti_aug")
    return str(root), make_kitti(str(root), frames=5, size=(37, 61))


def _batch_frames(r, content):
    frames = []
    for pi, sw in zip(r.last_pairs, r.last_swapped):
        p1, p2 = r.data_info[pi]
        if sw:
            p1, p2 = p2, p1
        frames.append((content[p1], content[p2]))
    return frames


def test_async_reader_augmented_bit_exact(kitti_tree):
    from optical_flow_amd.data_reader import AsyncReader, AugmentOpts, ReaderOpts, sample_augment
    root, content = kitti_tree
    aug = AugmentOpts(zoom=(1.0, 1.5), hflip_prob=0.5, rotate_deg=8.0, brightness=0.1,
                      contrast=(0.8, 1.2), saturation=(0.7, 1.3), color_gain=(0.9, 1.1))
    opts = ReaderOpts(root, 4, 48, 64, 4, seed=3, nslots=2, augment=aug)
    with AsyncReader(opts) as r:
        assert r.pinned and r.last_augment is None
        seen = []
        for k in range(2 * r.nbatches + 1):                    # crosses two epoch wraps
            batch = r.get_batch()
            rec = r.last_augment
            assert rec.tobytes() == sample_augment(aug, 4, 48, 64, 3, k).tobytes()
            exp = A.augment_pairs(_batch_frames(r, content), 48, 64, rec)
            np.testing.assert_array_equal(batch.cpu().numpy(), exp, err_msg="batch %d" % k)
            seen.append(rec.tobytes())
        assert len(set(seen)) == len(seen)                     # every batch its own draw


def test_reader_without_augment_is_the_plain_path(kitti_tree):
    from optical_flow_amd.data_reader import AsyncReader, ReaderOpts
    root, content = kitti_tree
    with AsyncReader(ReaderOpts(root, 4, 48, 64, 4, seed=3, nslots=2, augment=None)) as r:
        for _ in range(r.nbatches + 1):
            batch = r.get_batch()
            assert r.last_augment is None
            np.testing.assert_array_equal(batch.cpu().numpy(),
                                          D.preprocess_pairs(_batch_frames(r, content), 48, 64))


def test_train_driver_with_augment(tmp_path):
    from test_data_path import make_kitti
    from optical_flow_amd.train import main
    root = tmp_path / "kitti"
    make_kitti(str(root), days=(("2011_09_26", 2),), frames=6, size=(40, 130))
    log = tmp_path / "log.jsonl"
    main(["--kitti", str(root), "--height", "32", "--width", "64", "--batch", "2", "--epochs", "1",
          "--nworkers", "2", "--augment", "--aug-rotate", "5", "--log", str(log)])
    lines = [json.loads(l) for l in open(log).read().splitlines() if l]
    head, steps = lines[0], lines[1:]
    assert head["header"] is True and "step" not in head
    assert head["augment"] == {"zoom": [1.0, 1.3], "translate": True, "hflip_prob": 0.5,
                               "rotate_deg": 5.0, "brightness": 0.1, "contrast": [0.8, 1.2],
                               "saturation": [0.8, 1.2], "color_gain": [0.9, 1.1]}
    assert len(steps) == (2 * (5 + 6)) // 2
    assert all(np.isfinite(s["loss"]) for s in steps)


def test_argument_checks(lib):
    buf = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    out = torch.full((1, 2, 2, 6), 7.0, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    o = C.c_void_p(out.data_ptr())
    for args in [(p, 1, 2, 2, None, o, None),        # null dev_params
                 (p, 1, 0, 2, p, o, None),           # out_h = 0
                 (p, 1, 2, 0, p, o, None), (None, 1, 2, 2, p, o, None), (p, 1, 2, 2, p, None, None),
                 (p, -1, 2, 2, p, o, None), (p, 65536, 2, 2, p, o, None)]:
        assert lib.of_augment_pairs(*args) == 1                   # OF_EINVAL
        assert b"augment_pairs" in lib.of_last_error()
    assert lib.of_reader_next_aug(None, p, 1024, p, p, o, 2, 2, None, None, None) == 1
    assert b"reader_next_aug" in lib.of_last_error()
    torch.cuda.synchronize()
    assert (out == 7.0).all().item()                              # no kernel ran
