"""Labelled augmentation on the GPU (gt_augment.hip, ops.augment_gt, KittiFlowReader(...,
label_augment=...)): the kernel against the fp32 restatement bit for bit, its consistency with
the dense path (transform_flow) and with the supervised loss, and the reader end to end."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import gt_augment_ref as G
import kitti_flow_np as K
from helpers import dev
from optical_flow_amd._lib import call

pytestmark = pytest.mark.gpu

NAMES = ["identity", "flip", "zoom", "rotate", "preset1", "preset2"]
DESC = np.dtype([("offset", np.int64), ("h", np.int32), ("w", np.int32)])


def _pack_at(maps, offsets):
    """pack_gt_raw's layout with the maps at the given byte offsets."""
    desc = np.zeros(len(maps), DESC)
    end = max(o + m.nbytes for o, m in zip(offsets, maps))
    raw = np.zeros(-(-end // 256) * 256, np.uint8)
    for i, (o, m) in enumerate(zip(offsets, maps)):
        desc[i] = (o, m.shape[0], m.shape[1])
        raw[o:o + m.nbytes] = m.reshape(-1).view(np.uint8)
    raw[:16 * len(maps)] = desc.view(np.uint8)
    return raw, desc


def _split(raw, desc):
    """The maps of a raw ground-truth buffer (numpy)."""
    return [raw[d["offset"]:d["offset"] + 6 * d["h"] * d["w"]].copy().view(np.uint16)
            .reshape(d["h"], d["w"], 3) for d in desc]


def _run(gt, recs, img_hw=G.IMG_HW):
    from optical_flow_amd import ops
    out, desc = ops.augment_gt(gt, recs, img_hw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), desc


# ------------------------------------------------------- 1. against the restatement ----
@pytest.mark.parametrize("name", NAMES)
def test_kernel_matches_the_float32_restatement_bitwise(name):
    """The three sizes in one launch, largest first: 37 x 83 = 3071 pixels are 383 groups of
    eight (two workgroups) and a tail of seven, the groups straddle rows at every size (83, 14
    and 12 are no multiples of eight), and the small maps leave most of the grid idle."""
    order = [2, 0, 1]
    maps = [G.maps()[i] for i in order]
    recs = G.record_sets()[name][order]
    want = [G.reference(name)[i] for i in order]
    raw, desc = _run(maps, recs)
    again, _ = _run(maps, recs)
    got = _split(raw, desc)
    for i, (g, w) in enumerate(zip(got, want)):
        bad = int((g != w).any(-1).sum())
        print("%s map %d (%d x %d): %d valid pixels, %d differ" %
              (name, i, g.shape[0], g.shape[1], int((w[..., 2] != 0).sum()), bad))
        assert np.array_equal(g, w)
    assert np.array_equal(raw[:48].view(DESC), desc)              # the descriptors, copied
    assert all(np.array_equal(a, b) for a, b in zip(got, _split(again, desc)))


@pytest.mark.parametrize("name", ["zoom", "preset1"])
def test_maps_at_unaligned_offsets(name):
    """Offsets 4, 10 and 14 past a 16-byte boundary (heads of 2, 1 and 3 pixels before the first
    aligned group; the 7 x 12 map then has a tail too), an odd offset (byte stores), and an
    aligned map behind them."""
    idx = [2, 1, 0, 1, 2]
    maps = [G.maps()[i] for i in idx]
    recs = G.record_sets()[name][idx]
    offsets, at = [], 256
    for m, extra in zip(maps, (4, 10, 14, 1, 0)):
        offsets.append(at + extra)
        at = -(-(at + extra + m.nbytes) // 256) * 256
    raw, desc = _pack_at(maps, offsets)
    # the C entry itself, into a zeroed buffer, so that a write outside a map would show
    src = dev(torch.from_numpy(raw))
    prm = dev(torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8)))
    dst = torch.zeros_like(src)
    call("of_gt_augment", C.c_void_p(src.data_ptr()), desc.ctypes.data_as(C.c_void_p), src.numel(),
         len(maps), G.IMG_HW[0], G.IMG_HW[1], C.c_void_p(prm.data_ptr()),
         C.c_void_p(dst.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    for i, g in enumerate(_split(out, desc)):
        want = G.gt_augment_f32(maps[i], recs[i], G.IMG_HW)
        print("%s map %d at offset %d: %d differ" % (name, i, offsets[i],
                                                    int((g != want).any(-1).sum())))
        assert np.array_equal(g, want)
    assert np.array_equal(out[:16 * len(maps)].view(DESC), desc)
    gaps = np.ones(out.size, bool)                 # nothing is written ahead of a map or behind it
    gaps[:16 * len(maps)] = False
    for d in desc:
        gaps[d["offset"]:d["offset"] + 6 * d["h"] * d["w"]] = False
    assert gaps.any() and not out[gaps].any()
    # and through the op, whose output buffer is not zeroed
    got, _ = _run((src, desc), recs)
    assert all(np.array_equal(a, b) for a, b in zip(_split(got, desc), _split(out, desc)))


def test_degenerate_records_and_the_16_bit_range():
    H, W = G.IMG_HW
    rgb = np.ones((6, 8, 3), np.uint16)
    rgb[..., 0] = 32768 + 64 * 300
    rgb[..., 1] = 32768
    rgb[2, 3, 0] = 32768 + 64 * 400
    rgb[4, 5, 1] = 32768 - 64 * 400
    big = G.maps()[2]
    nan = float("nan")
    maps = [big, big, big, rgb, big]
    recs = np.array([G.zero(), G.record([nan] * 6), G.record([1.0 / W, 0, nan, 0, 1.0 / H, 0]),
                     G.zoom(H, W, 1.3), G.record([float("inf"), 0, 0, 0, 1.0 / H, 0])],
                    G.AUGMENT_DTYPE)
    raw, desc = _run(maps, recs)
    got = _split(raw, desc)
    for i in (0, 1, 2, 4):
        assert not got[i].any()
    want = G.gt_augment_f32(rgb, recs[3], G.IMG_HW)
    assert np.array_equal(got[3], want)
    assert int((want[..., 2] == 0).sum()) > 0 and not got[3][want[..., 2] == 0].any()


# ---------------------------------------------------------- 2. the dense path ----
FH, FW = 8, 16
NATIVE = np.array([[12.0, -5.0], [-7.25, 3.5], [20.015625, 9.984375]])     # px, on the 1/64 grid


def _constant_flows(fh, fw, native=NATIVE):
    """(3, fh, fw, 2) float32: per image the constant flow that is ``native`` in pixels of its
    map of G.SIZES."""
    f = np.empty((3, fh, fw, 2), np.float32)
    for i, (gh, gw) in enumerate(G.SIZES):
        f[i] = native[i] * np.array([fw / gw, fh / gh])
    return f


def _flip_zoom_records():
    H, W = G.IMG_HW
    return np.array([G.flip(H, W), G.zoom(H, W, 1.3, tx=0.3, ty=0.8),
                     G.zoom(H, W, 1.2, tx=0.6, ty=0.1, hflip=True)], G.AUGMENT_DTYPE)


def _mapped_native(recs):
    """A^-1 native per image, float64, A the record's linear part in native pixels."""
    H, W = G.IMG_HW
    out = []
    for i, (gh, gw) in enumerate(G.SIZES):
        m = np.asarray(recs[i]["m"], np.float64)
        A = np.array([[m[0] * W, m[1] * H * gw / gh], [m[3] * W * gh / gw, m[4] * H]])
        out.append(np.linalg.solve(A, NATIVE[i]))
    return np.array(out)


def _encoded_maps(sparse):
    """encode(upsample_flow(f)) per image at G.SIZES; ``sparse``: about 30 % of the pixels valid."""
    from optical_flow_amd.evaluate import encode_flow_kitti, upsample_flow
    f = dev(torch.from_numpy(_constant_flows(FH, FW)))
    rng = np.random.default_rng(41)
    maps = []
    for i, (gh, gw) in enumerate(G.SIZES):
        up = upsample_flow(f[i:i + 1], gh, gw)[0].cpu().numpy()
        valid = rng.uniform(size=(gh, gw)) < 0.3 if sparse else None
        maps.append(encode_flow_kitti(up, valid))
    return f, maps


def test_consistent_with_transform_flow():
    """A constant flow carried densely (transform_flow) and as encoded sparse truth
    (augment_gt) must agree to the output's quantisation: the native vectors lie on the 1/64
    grid, so encoding them loses nothing, and the carried truth is rounded once, by at most
    1/128 px per channel."""
    from optical_flow_amd import ops
    from optical_flow_amd.evaluate import flow_metrics
    recs = _flip_zoom_records()
    f, maps = _encoded_maps(sparse=False)
    target, weight = ops.transform_flow(f, recs, G.IMG_HW)
    gt = ops.augment_gt(maps, recs, G.IMG_HW)
    s, v, _ = flow_metrics(target, *gt)
    s, v = s.cpu().numpy(), v.cpu().numpy()
    for i, (gh, gw) in enumerate(G.SIZES):
        print("image %d: %d of %d pixels valid, mean EPE %.5f px" % (i, v[i], gh * gw, s[i] / v[i]))
        assert v[i] == gh * gw                     # a crop inside the frame loses no pixel
        assert s[i] / v[i] <= 1.0 / 64.0


def test_the_supervised_loss_sees_the_carried_truth():
    from optical_flow_amd import ops
    recs = _flip_zoom_records()
    _, maps = _encoded_maps(sparse=True)
    gt = ops.augment_gt(maps, recs, G.IMG_HW)
    grids = [(8, 16), (4, 8), (2, 4)]
    mapped = [dev(torch.from_numpy(_constant_flows(fh, fw, _mapped_native(recs))))
              for fh, fw in grids]
    plain = [dev(torch.from_numpy(_constant_flows(fh, fw))) for fh, fw in grids]
    good = ops.supervised_flow_loss(mapped, gt, q=1.0, eps=0.01).item()
    bad = ops.supervised_flow_loss(plain, gt, q=1.0, eps=0.01).item()
    print("supervised loss against the carried truth: mapped flows %.5f, un-mapped %.3f"
          % (good, bad))
    assert good <= 0.02 and bad > 1.0


# ---------------------------------------------------------- 3. the reader ----
H, W = 64, 128


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """Five tiny labelled frames of two native sizes in KITTI's layout."""
    root = str(tmp_path_factory.mktemp("kitti_flow_aug_gpu"))
    tr = os.path.join(root, "training")
    for d in ("image_2", "flow_occ"):
        os.makedirs(os.path.join(tr, d))
    rng = np.random.default_rng(9)
    for k in range(5):
        h, w = ((9, 14), (7, 12))[k % 2]
        for rel in ("image_2/%06d_10.png", "image_2/%06d_11.png"):
            K.write_png(os.path.join(tr, rel % k), rng.integers(0, 256, (h, w, 3)).astype(np.uint8))
        K.write_png(os.path.join(tr, "flow_occ/%06d_10.png" % k), G.make_map(h, w, rng, mag=4.0))
    return root


def test_reader_end_to_end(tree):
    from optical_flow_amd.data_reader import augment_frames
    from optical_flow_amd.evaluate import KittiFlowReader
    from optical_flow_amd.loss import LossLayer
    from optical_flow_amd.model import build_flow_net
    from optical_flow_amd.train import Trainer
    reader = KittiFlowReader(tree, 2, H, W, seed=3, nworkers=2, label_augment=G.preset_opts())
    last = None
    for epoch in range(2):
        host = list(reader.host_batches(epoch))
        got = list(reader)
        assert len(got) == len(host) == reader.nbatches == 2
        for k, ((batch, gt_raw, descs), (pairs, maps, _)) in enumerate(zip(got, host)):
            recs = reader.records(epoch, k)
            want = augment_frames(pairs, H, W, recs)
            assert torch.equal(batch, want)
            out = _split(gt_raw.cpu().numpy(), descs)
            for i, m in enumerate(maps):
                assert np.array_equal(out[i], G.gt_augment_f32(m, recs[i], (H, W)))
            last = (batch, gt_raw, descs)
    assert reader.epoch == 2
    net = build_flow_net(H, W, seed=0, levels=4, warp_convention="image")
    trainer = Trainer(net, loss_layer=LossLayer(warp_convention="image", photometric_weight=0.0,
                                                supervised_weight=1.0))
    net.store.zero_grad()
    batch, gt_raw, descs = last
    loss, _ = trainer.train_step(batch, gt=(gt_raw, descs))
    torch.cuda.synchronize()
    grads = net.store.grad_arena
    print("augmented labelled step: loss %.5f, |grad| %.3e" % (loss.item(), grads.norm().item()))
    assert np.isfinite(loss.item()) and bool(torch.isfinite(grads).all()) and bool(grads.any())


def test_reader_without_label_augment_launches_no_new_kernel(tree):
    from optical_flow_amd import evaluate, ops
    from optical_flow_amd.data_reader import preprocess_frames
    reader = evaluate.KittiFlowReader(tree, 2, H, W, seed=3, nworkers=2)
    called = []
    real_e, real_o = evaluate.call, ops.call
    evaluate.call = lambda name, *a: (called.append(name), real_e(name, *a))[1]
    ops.call = lambda name, *a: (called.append(name), real_o(name, *a))[1]
    try:
        got = list(reader)
    finally:
        evaluate.call, ops.call = real_e, real_o
    # the PNG decodes and the parent's one kernel, nothing else
    assert set(called) == {"of_png_info", "of_png_read_u16", "of_preprocess_pairs"}
    for (batch, gt_raw, descs), (pairs, maps, _) in zip(got, reader.host_batches(0)):
        assert torch.equal(batch, preprocess_frames(pairs, H, W))
        assert all(np.array_equal(a, b) for a, b in zip(_split(gt_raw.cpu().numpy(), descs), maps))
