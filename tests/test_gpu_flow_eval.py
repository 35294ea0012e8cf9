"""The KITTI flow evaluation on the GPU: of_flow_eval / of_flow_upsample (flow_eval.hip) against
the float64 restatement of tests/kitti_flow_np.py, their meaning pinned on inputs whose result
is known analytically, and evaluate() / predict_flow() end to end on a small KITTI-format tree
written with the independent PNG writer.

Tolerance: 2e-4 px on the mean EPE and on each upsampled component, for |flow| <= 256 px: an
fp32 ulp there is <= 3.1e-5, the sample is three roundings of lerp plus one scale and one
subtraction per component, and the sum is in double.  The counts must be EQUAL: the inputs
keep every valid pixel >= 0.1 px from the 3 px threshold and >= 1e-3 from the 5 % ratio (asserted
on the restatement for every valid pixel), three orders above that error."""
import os

import numpy as np
import pytest
import torch

import kitti_flow_np as K
from helpers import dev

pytestmark = pytest.mark.gpu

TOL = 2e-4

# name -> (fh, fw, the batch's ground-truth sizes, seed)
CASES = {
    "three_sizes": (8, 16, [(37, 61), (33, 67), (13, 21)], 1),   # odd widths, descriptor path
    "wide": (12, 20, [(47, 125)], 2),
    "one_cell_grid": (1, 1, [(5, 7)], 3),                        # every clamp active
    "one_pixel_map": (4, 4, [(1, 1)], 8),
    "full_size": (96, 320, [(375, 1242)] * 2, 5),                # 114 partials per image
}
_cache = {}


def case(name):
    """(flow, maps, the restatement's sums), computed once per session and never modified."""
    if name not in _cache:
        fh, fw, sizes, seed = CASES[name]
        flow, maps = K.make_case(fh, fw, sizes, seed)
        _cache[name] = (flow, maps, K.flow_eval_np(flow, maps), K.margins_np(flow, maps))
    return _cache[name]


def run_eval(flow, gt, descs=None):
    from optical_flow_amd.evaluate import flow_metrics
    s, v, o = flow_metrics(dev(torch.from_numpy(flow)), gt, descs)
    return s.cpu().numpy(), v.cpu().numpy(), o.cpu().numpy()


def check_against(ref, got, what=""):
    (rs, rv, ro), (s, v, o) = ref, got
    assert s.dtype == np.float64 and v.dtype == np.int64 and o.dtype == np.int64
    for i in range(len(rv)):
        mean_ref = rs[i] / max(rv[i], 1)
        mean = s[i] / max(v[i], 1)
        print("%s image %d: n_valid %d / %d, n_outlier %d / %d, mean EPE %.7f / %.7f (diff %.2e)" %
              (what, i, v[i], rv[i], o[i], ro[i], mean, mean_ref, abs(mean - mean_ref)))
    np.testing.assert_array_equal(v, rv)
    np.testing.assert_array_equal(o, ro)
    np.testing.assert_allclose(s / np.maximum(v, 1), rs / np.maximum(rv, 1), rtol=0, atol=TOL)


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_matches_restatement(name):
    from optical_flow_amd.evaluate import upsample_flow
    flow, maps, ref, (m3, m5) = case(name)
    # the input, not the kernel: within the tolerance's range (native |flow| <= 256 px, ground
    # truth included: 190 + 20), and no valid pixel near a threshold
    for f, rgb in zip(flow, maps):
        scale = np.array([rgb.shape[1] / f.shape[1], rgb.shape[0] / f.shape[0]])
        assert np.abs(f * scale).max() <= 200.0
    assert m3 >= 0.1 and m5 >= 1e-3, (m3, m5)
    got = run_eval(flow, maps)
    check_against(ref, got, name)
    if name != "one_pixel_map":
        assert ref[1].sum() > 0
    # two runs: bitwise equal
    again = run_eval(flow, maps)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    # of_flow_upsample: the restatement's (u, v), and the same counts from its output
    for i, rgb in enumerate(maps):
        gh, gw = rgb.shape[:2]
        up = upsample_flow(dev(torch.from_numpy(flow[i:i + 1])), gh, gw)
        assert up.shape == (1, gh, gw, 2) and up.dtype == torch.float32
        up = up[0].cpu().numpy()
        err = np.abs(up - K.upsample_np(flow[i], gh, gw)).max()
        print("%s image %d: upsample max |diff| %.2e" % (name, i, err))
        assert err <= TOL
        epe, _, valid, outlier = K.epe_np(up, rgb)
        assert int(valid.sum()) == got[1][i] and int(outlier.sum()) == got[2][i]


def test_one_pixel_map_with_a_valid_pixel():
    """The recipe's 1 x 1 map samples the blend band between the flow's halves, which it marks
    invalid; here the one pixel is valid, 3.5 px and then 20 px from the upsampled flow."""
    flow = K.make_case(4, 4, [(1, 1)], 8)[0]
    up = K.upsample_np(flow[0], 1, 1)
    for err in (3.5, 20.0):
        rgb = np.ones((1, 1, 3), np.uint16)
        rgb[0, 0, :2] = np.rint((up[0, 0] + (err, 0.0)) * 64.0) + 32768
        m3, m5 = K.margins_np(flow, [rgb])
        assert m3 >= 0.1 and m5 >= 1e-3, (m3, m5)
        ref = K.flow_eval_np(flow, [rgb])
        assert ref[1][0] == 1
        check_against(ref, run_eval(flow, [rgb]), "1 x 1, err %g" % err)


def test_upsample_of_a_batch():
    from optical_flow_amd.evaluate import upsample_flow
    flow = K.make_case(8, 16, [(21, 35)] * 3, 4)[0]
    up = upsample_flow(dev(torch.from_numpy(flow)), 21, 35).cpu().numpy()
    for i in range(3):
        assert np.abs(up[i] - K.upsample_np(flow[i], 21, 35)).max() <= TOL


@pytest.mark.parametrize("shift", [2, 6, 1], ids=["plus2", "plus6", "odd"])
def test_maps_at_unaligned_offsets(shift):
    """A map whose offset is not 16-byte aligned is read byte by byte: the same sums."""
    from optical_flow_amd.evaluate import DESC_DTYPE
    flow, maps, ref, _ = case("three_sizes")
    n = len(maps)
    desc = np.zeros(n, DESC_DTYPE)
    total = 256
    for i, m in enumerate(maps):
        desc[i] = (total + shift, m.shape[0], m.shape[1])
        total += -(-(m.nbytes + shift) // 256) * 256
    raw = np.zeros(total, np.uint8)
    raw[:16 * n] = desc.view(np.uint8)
    for d, m in zip(desc, maps):
        raw[d["offset"]:d["offset"] + m.nbytes] = m.reshape(-1).view(np.uint8)
    check_against(ref, run_eval(flow, raw, desc), "shift %d" % shift)


def test_constant_flow_and_channel_meaning():
    """A constant flow (a, b) on the flow grid is the constant (a gw/fw, b gh/fh) in native
    pixels: against exactly that ground truth EPE = 0 with no outlier; with the ground truth's
    x and y swapped the error is known, which pins channel 0 to R and x."""
    fh, fw, gh, gw = 8, 16, 32, 48                       # gw / fw = 3, gh / fh = 4
    a, b = 1.5, -2.25                                    # -> (4.5, -9.0): multiples of 1/64
    flow = np.broadcast_to(np.array([a, b], np.float32), (2, fh, fw, 2)).copy()
    gu, gv = a * gw / fw, b * gh / fh
    right = np.zeros((gh, gw, 3), np.uint16)
    right[:, :, 0] = int(gu * 64) + 32768
    right[:, :, 1] = int(gv * 64) + 32768
    right[:, :, 2] = 1
    swapped = right.copy()
    swapped[:, :, 0], swapped[:, :, 1] = right[:, :, 1], right[:, :, 0]
    s, v, o = run_eval(flow, [right, swapped])
    assert v.tolist() == [gh * gw, gh * gw]
    assert s[0] == 0.0 and o[0] == 0
    expect = np.sqrt(2.0) * abs(gu - gv)                 # |(gu - gv, gv - gu)| = 19.09 px
    assert abs(s[1] / v[1] - expect) <= TOL and o[1] == gh * gw
    # a zero ground truth with epe > 3 is an outlier; under 3 px it is not
    zero = right.copy()
    zero[:, :, :2] = 32768
    s, v, o = run_eval(flow, [zero, zero])
    assert o.tolist() == [gh * gw] * 2 and abs(s[0] / v[0] - np.hypot(gu, gv)) <= TOL
    small = np.broadcast_to(np.array([0.5, 0.25], np.float32), (1, fh, fw, 2)).copy()
    s, v, o = run_eval(small, [zero])
    assert o[0] == 0 and abs(s[0] / v[0] - np.hypot(1.5, 1.0)) <= TOL


def test_all_invalid_image_counts_nothing():
    flow, maps, ref, _ = case("three_sizes")
    blank = [maps[0], np.zeros_like(maps[1]), maps[2]]
    blank[1][:, :, :2] = 40000                           # samples, but B = 0 everywhere
    s, v, o = run_eval(flow, blank)
    assert v[1] == 0 and o[1] == 0 and s[1] == 0.0
    assert v[0] == ref[1][0] and v[2] == ref[1][2]


# ---- end to end -------------------------------------------------------------------------------
H, W = 64, 128
SIZES = [(40, 70), (37, 71), (43, 66)]


def _net(convention="image"):
    from optical_flow_amd.model import FlowNet
    from optical_flow_amd.params import flow_net_spec, init_params, perturb_params
    return FlowNet(H, W, warp_convention=convention,
                   values=perturb_params(init_params(flow_net_spec(), 0), 1))


class Tree:
    pass


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """Three frames of different native sizes in KITTI's layout: random 8-bit images, ground
    truth built (K.make_gt) around the net's own prediction so that the metric has every
    branch to take; plus a fourth frame, outside the tree, without a valid pixel."""
    from optical_flow_amd.data_reader import preprocess_frames
    t = Tree()
    t.root = str(tmp_path_factory.mktemp("kitti_flow"))
    tr = os.path.join(t.root, "training")
    for d in ("image_2", "flow_occ"):
        os.makedirs(os.path.join(tr, d))
    rng = np.random.default_rng(11)
    t.net = _net()
    t.pairs, t.maps, t.frames = [], [], []
    for k, (h, w) in enumerate(SIZES):
        rgb1 = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        rgb2 = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        trio = tuple(os.path.join(tr, rel % k) for rel in
                     ("image_2/%06d_10.png", "image_2/%06d_11.png", "flow_occ/%06d_10.png"))
        K.write_png(trio[0], rgb1, filt=k)
        K.write_png(trio[1], rgb2, filt="cycle")
        t.pairs.append((rgb1[:, :, ::-1].copy(), rgb2[:, :, ::-1].copy()))     # BGR, as decoded
        t.frames.append(trio)
    # the flows evaluate(batch_size=2) will see: net(batch) of frames 0-1, then of frame 2
    with torch.no_grad():
        t.flows = [t.net(preprocess_frames(t.pairs[:2], H, W))[0].cpu().numpy(),
                   t.net(preprocess_frames(t.pairs[2:], H, W))[0].cpu().numpy()]
    t.flows = np.concatenate(t.flows)
    assert t.flows.shape == (3, H // 2, W // 2, 2)
    for k, (h, w) in enumerate(SIZES):
        gmap = K.make_gt(K.upsample_np(t.flows[k], h, w), rng)
        K.write_png(t.frames[k][2], gmap, filt=(k + 2) % 5)
        t.maps.append(gmap)
    t.empty = os.path.join(t.root, "empty_10.png")
    K.write_png(t.empty, np.zeros((SIZES[0][0], SIZES[0][1], 3), np.uint16))
    return t


def test_evaluate_end_to_end(tree):
    from optical_flow_amd.evaluate import evaluate
    m3, m5 = K.margins_np(tree.flows, tree.maps)
    assert m3 >= 0.1 and m5 >= 1e-3, (m3, m5)
    rs, rv, ro = K.flow_eval_np(tree.flows, tree.maps)
    assert (rv > 0).all()
    version = tree.net.store.version
    grads = tree.net.store.grad_arena.clone()
    res = evaluate(tree.net, tree.root, batch_size=2)            # batches of 2 and 1
    assert tree.net.store.version == version
    assert torch.equal(tree.net.store.grad_arena, grads)
    per = res["per_image"]
    check_against((rs, rv, ro), (per["sum_epe"], per["n_valid"], per["n_outlier"]), "tree")
    assert res["n_images"] == 3 and res["n_images_empty"] == 0 and res["n_valid"] == rv.sum()
    assert abs(res["epe"] - np.mean(rs / rv)) <= TOL
    assert abs(res["fl_all"] - np.mean(100.0 * ro / rv)) <= 1e-9
    assert abs(res["epe_pooled"] - rs.sum() / rv.sum()) <= TOL
    assert abs(res["fl_pooled"] - 100.0 * ro.sum() / rv.sum()) <= 1e-9
    # the same from a frame list, and with the other batch split (one batch of 3)
    res3 = evaluate(tree.net, tree.frames, batch_size=8, nworkers=1)
    check_against((rs, rv, ro), tuple(res3["per_image"][k] for k in
                                      ("sum_epe", "n_valid", "n_outlier")), "one batch")


def test_evaluate_leaves_empty_images_out_of_the_means(tree):
    from optical_flow_amd.evaluate import evaluate
    f0 = tree.frames[0]
    res = evaluate(tree.net, [f0, (f0[0], f0[1], tree.empty)], batch_size=2)
    per = res["per_image"]
    assert per["n_valid"][1] == 0 and per["n_outlier"][1] == 0 and per["sum_epe"][1] == 0.0
    assert res["n_images"] == 2 and res["n_images_empty"] == 1
    assert np.isfinite(res["epe"]) and np.isfinite(res["fl_all"])
    assert res["epe"] == per["sum_epe"][0] / per["n_valid"][0]
    assert res["epe_pooled"] == res["epe"]


def test_predict_flow_is_the_upsampled_finest_flow(tree):
    from optical_flow_amd.data_reader import preprocess_frames
    from optical_flow_amd.evaluate import predict_flow, upsample_flow
    h, w = SIZES[0]
    pred = predict_flow(tree.net, *tree.pairs[0])
    assert pred.shape == (h, w, 2) and pred.dtype == torch.float32 and not pred.requires_grad
    with torch.no_grad():
        flow = tree.net(preprocess_frames(tree.pairs[:1], H, W))[0]
    assert torch.equal(pred, upsample_flow(flow, h, w)[0])
    # and it is the flow evaluate() scored (the batch of two's first image), within rounding
    assert np.abs(pred.cpu().numpy() - K.upsample_np(tree.flows[0], h, w)).max() <= 1e-3


@pytest.mark.parametrize("fmt", ["tf", "npz"])
def test_command_line_loads_the_whole_checkpoint(tree, tmp_path, capsys, fmt):
    """`python -m optical_flow_amd.evaluate --weights CKPT` scores the saved net, every tensor of
    it: its JSON line equals evaluate() on the in-memory net that was saved, for a TensorFlow
    checkpoint prefix (what train --save-dir writes) and for an .npz."""
    import json
    from optical_flow_amd import evaluate as E
    path = str(tmp_path / "ckpt" / ("weights.npz" if fmt == "npz" else "weights"))
    tree.net.save_weights(path)
    want = E.evaluate(tree.net, tree.root, batch_size=2)
    capsys.readouterr()
    E.main(["--kitti-flow", tree.root, "--weights", path, "--height", str(H), "--width", str(W),
            "--batch", "2", "--seed", "5"])          # another seed: nothing of the initial net stays
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    got = json.loads(lines[0])
    for key in ("epe", "fl_all", "epe_pooled", "fl_pooled", "n_images", "n_images_empty",
                "n_valid", "per_image"):
        assert key in got, key
    assert got["per_image"]["n_valid"] == want["per_image"]["n_valid"].tolist()
    assert got["per_image"]["n_outlier"] == want["per_image"]["n_outlier"].tolist()
    np.testing.assert_allclose(got["per_image"]["sum_epe"], want["per_image"]["sum_epe"],
                               rtol=1e-9, atol=0)
    assert got["epe"] == pytest.approx(want["epe"], rel=1e-9)
    assert got["fl_all"] == pytest.approx(want["fl_all"], rel=1e-12)
    # and it is not the seeded initial net's score
    init = E.evaluate(_seeded_net(5), tree.root, batch_size=2)
    assert abs(init["epe"] - want["epe"]) > 1e-3


def test_command_line_refuses_a_partial_checkpoint(tree, tmp_path):
    """A file that lacks any of the net's tensors (here: the encoder's alone, what
    build_flow_net's pretrained path takes) is an error, not a half-loaded net."""
    from optical_flow_amd import evaluate as E
    from optical_flow_amd.params import encoder_spec
    names = {p.name for p in encoder_spec(4)}
    state = tree.net.store.state()
    assert 0 < len(names) < len(state)
    path = str(tmp_path / "encoder_only.npz")
    np.savez(path, **{k: v for k, v in state.items() if k in names})
    with pytest.raises(KeyError, match="missing"):
        E.main(["--kitti-flow", tree.root, "--weights", path, "--height", str(H), "--width",
                str(W)])
    with pytest.raises(FileNotFoundError):
        E.main(["--kitti-flow", tree.root, "--weights", str(tmp_path / "nothing"), "--height",
                str(H), "--width", str(W)])


def _seeded_net(seed):
    from optical_flow_amd.model import FlowNet
    return FlowNet(H, W, warp_convention="image", seed=seed)


def test_reference_convention_is_refused(tree):
    from optical_flow_amd.evaluate import evaluate, predict_flow
    net = _net("reference")
    with pytest.raises(ValueError, match="image"):
        evaluate(net, tree.root, batch_size=2)
    with pytest.raises(ValueError, match="image"):
        predict_flow(net, *tree.pairs[0])


def test_graphed_step_replays_after_an_evaluate(tree):
    """A train step captured before an evaluate() call replays after it as on a twin trainer
    that never evaluated: same loss, same updated weights (deterministic warp backward, so the
    comparison is bitwise)."""
    from optical_flow_amd import ops
    from optical_flow_amd.data import synthetic_batch
    from optical_flow_amd.evaluate import evaluate
    from optical_flow_amd.train import KerasAdam, Trainer
    batch = torch.from_numpy(synthetic_batch(2, H, W, seed=77))

    def run(with_eval):
        net = _net()
        trainer = Trainer(net, KerasAdam(net.store, learning_rate=1e-4))
        step = trainer.graphed(dev(batch.clone()), warmup=1)
        if with_eval:
            version = net.store.version
            res = evaluate(net, tree.root, batch_size=2)
            assert res["n_images"] == 3 and net.store.version == version
        loss, _ = step()
        torch.cuda.synchronize()
        return float(loss), net.store.arena.clone()

    with ops.deterministic(True):
        loss_a, w_a = run(True)
        loss_b, w_b = run(False)
    print("replay loss after evaluate %.9e, twin %.9e" % (loss_a, loss_b))
    assert loss_a == loss_b
    assert torch.equal(w_a, w_b)
