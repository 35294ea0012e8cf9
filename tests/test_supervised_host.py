"""The supervised term without a GPU: the conditioning of the GPU tests' inputs (an fp32
evaluation of the float64 restatement stays far inside the tolerance they use), the LossLayer /
train-command validation, the labelled reader's split and seeded order, the C entry's argument
checks, and that a default LossLayer calls ops exactly as before."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import kitti_flow_np as K
import supervised_ref as R
from helpers import REL_TOL, rel_l2


# ------------------------------------------------------------------ the reference ----
@pytest.mark.parametrize("name", list(R.CASES))
@pytest.mark.parametrize("q", R.QS)
def test_float32_reference_is_well_conditioned_on_the_gpu_inputs(name, q):
    flows, maps = R.case(name)
    v64, s64, g64 = R.reference(name, q)
    v32, s32, g32 = R.supervised_ref(flows, maps, q, R.EPS, dtype=torch.float32)
    assert abs(v32 - v64) <= REL_TOL / 10 * abs(v64)
    for l, (a, b) in enumerate(zip(g32, g64)):
        err = float(rel_l2(torch.from_numpy(a), torch.from_numpy(b)))
        print("%s q=%g level %d: fp32 vs float64 rel_l2 %.2e" % (name, q, l, err))
        assert err <= REL_TOL / 10
    # the inputs are what the issue asks for: native |flow| <= 48 px, about 30 % valid
    for f, in zip(flows[:1]):
        for i, rgb in enumerate(maps):
            scale = np.array([rgb.shape[1] / f.shape[2], rgb.shape[0] / f.shape[1]])
            assert np.sqrt(((f[i] * scale) ** 2).sum(-1)).max() <= 48.0 + 1e-3
    if maps[0].size > 3000:
        frac = np.mean([(m[:, :, 2] != 0).mean() for m in maps])
        assert 0.25 < frac < 0.35


def test_restatement_known_answers():
    # a constant flow c under ground truth exactly c * (gw / fw, gh / fh): eps^q, no gradient
    flow = np.full((1, 2, 4, 2), 0.5, np.float32)
    rgb = np.ones((6, 8, 3), np.uint16)
    rgb[:, :, 0] = 32768 + 64 * 1          # 0.5 * 8 / 4
    rgb[:, :, 1] = int(32768 + 64 * 1.5)   # 0.5 * 6 / 2
    for q in (1.0, 0.4):
        v, _, g = R.supervised_ref([flow], [rgb], q, 0.01)
        assert abs(v - 0.01 ** q) < 1e-15 and np.abs(g[0]).max() == 0.0
    rgb[:, :, 0] += 64 * 3
    rgb[:, :, 1] += 64 * 4
    v, _, _ = R.supervised_ref([flow], [rgb], 1.0, 0.01)
    assert abs(v - (25 + 1e-4) ** 0.5) < 1e-14
    # empty images: left out of the mean; all empty: 0
    empty = np.zeros((6, 8, 3), np.uint16)
    two = np.concatenate([flow, flow])
    assert abs(R.supervised_ref([two], [rgb, empty], 1.0, 0.01)[0] - v) < 1e-14
    v0, _, g0 = R.supervised_ref([two], [empty, empty], 1.0, 0.01)
    assert v0 == 0.0 and np.abs(g0[0]).max() == 0.0


# ------------------------------------------------------------------------ LossLayer ----
@pytest.mark.parametrize("kw", [
    dict(supervised_weight=-1.0), dict(supervised_weight=float("nan")),
    dict(supervised_weight=1.0),                                   # reference convention
    dict(supervised_weight=1.0, warp_convention="image", supervised_q=0.0),
    dict(supervised_weight=1.0, warp_convention="image", supervised_q=2.5),
    dict(supervised_weight=1.0, warp_convention="image", supervised_eps=0.0),
    dict(supervised_weight=1.0, warp_convention="image", supervised_level_weights=[1.0, -1.0]),
    dict(supervised_weight=1.0, warp_convention="image", supervised_level_weights=[]),
])
def test_loss_layer_rejects(kw):
    from optical_flow_amd.loss import LossLayer
    with pytest.raises(ValueError):
        LossLayer(**kw)


def test_loss_layer_data_weights_may_all_be_zero_with_the_supervised_term():
    from optical_flow_amd.loss import LossLayer
    d = LossLayer(photometric_weight=0.0, supervised_weight=1.0, warp_convention="image")
    assert (d.supervised_weight, d.supervised_q, d.supervised_eps) == (1.0, 1.0, 0.01)
    assert d.supervised_level_weights is None
    d = LossLayer(photometric_weight=0.0, supervised_weight=2.0, supervised_q=0.4,
                  supervised_level_weights=[0.5, 0.25], warp_convention="image", occlusion="fb")
    assert d.supervised_level_weights == (0.5, 0.25) and d.supervised_q == 0.4
    # without the term the "all 0" error and its text stay
    with pytest.raises(ValueError, match="census_weight, photometric_weight and ssim_weight are "
                                         "all 0: the loss needs a data term"):
        LossLayer(photometric_weight=0.0)
    assert LossLayer().supervised_weight == 0.0


def _fake_flows(n=2, h=64, w=128, levels=4):
    return [torch.zeros(n, h >> (k + 1), w >> (k + 1), 2) for k in range(levels)]


def test_loss_layer_call_needs_gt_exactly_when_the_term_is_on():
    from optical_flow_amd.loss import LossLayer
    imgs = torch.zeros(2, 64, 128, 6)
    with pytest.raises(ValueError, match="gt"):
        LossLayer(photometric_weight=0.0, supervised_weight=1.0,
                  warp_convention="image")(imgs, _fake_flows())
    with pytest.raises(ValueError, match="supervised_weight is 0"):
        LossLayer()(imgs, _fake_flows(), gt=[np.zeros((4, 4, 3), np.uint16)] * 2)
    with pytest.raises(ValueError, match="supervised_level_weights"):
        LossLayer(supervised_weight=1.0, warp_convention="image",
                  supervised_level_weights=[1.0, 1.0])(imgs, _fake_flows(),
                                                       gt=[np.zeros((4, 4, 3), np.uint16)] * 2)


@pytest.mark.parametrize("kw,entry", [
    (dict(), "photometric_loss"),
    (dict(smoothness_weight=0.5, edge_alpha=2.0), "flow_loss"),
    (dict(census_weight=1.0), "census_flow_loss"),
    (dict(photometric_weight=0.15, ssim_weight=0.85, smoothness_order=2,
          smoothness_weight=1.0), "census_flow_loss"),
])
def test_default_call_path_is_unchanged(monkeypatch, kw, entry):
    """Without the supervised term LossLayer calls the ops entry it always called, with the
    arguments it always passed: no supervised keyword, no gt."""
    from optical_flow_amd import ops
    from optical_flow_amd.loss import LossLayer
    calls = []
    for name in ("photometric_loss", "flow_loss", "census_flow_loss"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append((_n, a, k)) or "L")
    imgs, flows = torch.zeros(2, 64, 128, 6), _fake_flows()
    layer = LossLayer(**kw)
    assert layer(imgs, flows) == "L"
    (name, args, kwargs), = calls
    assert name == entry and args[0] is imgs
    assert all(a is b for a, b in zip(args[1], flows))
    assert not any(k.startswith("supervised") or k == "gt" for k in kwargs)
    want = {"photometric_loss": (imgs, flows, "reference"),
            "flow_loss": (imgs, flows, 0.5, 2.0, 1e-4, "reference")}
    if entry in want:
        assert args[2:] == want[entry][2:] and kwargs == {}
    elif "ssim_weight" in kw:
        assert args[2:] == (0.0, 3, 0.15, 1.0, 0.0, 1e-4, "reference")
        assert kwargs == {"smoothness_order": 2, "ssim_weight": 0.85}
    else:
        assert args[2:] == (1.0, 3, 1.0, 0.0, 0.0, 1e-4, "reference") and kwargs == {}


def test_supervised_call_passes_the_term_to_census_flow_loss(monkeypatch):
    from optical_flow_amd import ops
    from optical_flow_amd.loss import LossLayer
    seen = {}
    monkeypatch.setattr(ops, "census_flow_loss", lambda *a, **k: seen.update(k) or "L")
    monkeypatch.setattr(ops, "_gt_handle", lambda gt, n: ("handle", gt, n))
    layer = LossLayer(photometric_weight=0.0, supervised_weight=2.0, supervised_q=0.4,
                      warp_convention="image")
    assert layer(torch.zeros(2, 64, 128, 6), _fake_flows(), gt="maps") == "L"
    assert seen["supervised_weight"] == 2.0 and seen["supervised_q"] == 0.4
    assert seen["supervised_eps"] == 0.01 and seen["supervised_level_weights"] is None
    assert seen["gt"] == ("handle", "maps", 2) and "weights" not in seen
    # occlusion="fb": the ground truth belongs to the first half of the doubled batch
    monkeypatch.setattr(ops, "occlusion_masks", lambda *a, **k: ["m"] * 4)
    layer = LossLayer(supervised_weight=1.0, warp_convention="image", occlusion="fb")
    layer(torch.zeros(4, 64, 128, 6), _fake_flows(4), gt="maps")
    assert seen["gt"] == ("handle", "maps", 2) and seen["weights"] == ["m"] * 4


def test_ops_argument_checks():
    from optical_flow_amd import ops
    fl = _fake_flows()
    maps = [np.zeros((4, 4, 3), np.uint16)] * 2
    with pytest.raises(ValueError, match="q must be"):
        ops.supervised_flow_loss(fl, maps, q=3.0)
    with pytest.raises(ValueError, match="eps must be"):
        ops.supervised_flow_loss(fl, maps, eps=0.0)
    with pytest.raises(ValueError, match="ground truth"):
        ops.supervised_flow_loss(fl, None)
    with pytest.raises(ValueError, match="level weights"):
        ops.supervised_flow_loss(fl, maps, level_weights=[1.0])
    with pytest.raises(ValueError, match="supervised_weight is 0"):
        ops.census_flow_loss(None, fl, 0.0, gt=maps)
    with pytest.raises(ValueError, match="image warp convention"):
        ops.census_flow_loss(None, fl, 0.0, supervised_weight=1.0, gt=maps)
    with pytest.raises(RuntimeError, match="GPU only"):           # no CPU fall-back
        ops.supervised_flow_loss(fl, maps)


def test_evaluate_keeps_its_names():
    from optical_flow_amd import evaluate, gt_raw
    assert evaluate.pack_gt_raw is gt_raw.pack_gt_raw and evaluate._upload is gt_raw._upload
    assert evaluate.DESC_DTYPE is gt_raw.DESC_DTYPE


# -------------------------------------------------------------------- Trainer ----
def test_graphed_step_refuses_a_supervised_layer():
    from optical_flow_amd.loss import LossLayer
    from optical_flow_amd.train import GraphedStep

    class T:
        reducer = None
        loss_layer = LossLayer(supervised_weight=1.0, warp_convention="image")
    with pytest.raises(RuntimeError, match="supervised"):
        GraphedStep(T(), None)


# ------------------------------------------------------------------ train command ----
def _parse(argv):
    from optical_flow_amd.train import build_parser
    return build_parser().parse_args(argv)


def test_parser_defaults_and_header_record():
    from optical_flow_amd.train import header_record
    a = _parse([])
    assert (a.kitti_flow, a.kitti_flow_holdout, a.supervised_weight, a.supervised_q,
            a.supervised_eps) == (None, 0, 0.0, 1.0, 0.01)
    assert header_record(a) is None
    # the keys appear only when the term is on: other logs stay what they were
    assert header_record(_parse(["--ssim-weight", "0.5"])) == {
        "header": True, "smoothness_weight": 0.0, "edge_alpha": 0.0, "ssim_weight": 0.5}
    head = header_record(_parse(["--census-weight", "1", "--kitti-flow", "/x"]))
    assert not any(k.startswith("supervised") or k.startswith("kitti_flow") for k in head)
    head = header_record(_parse(["--kitti-flow", "/x", "--warp-convention", "image",
                                 "--photometric-weight", "0", "--supervised-weight", "1",
                                 "--supervised-q", "0.4", "--kitti-flow-holdout", "5"]))
    assert head["supervised_weight"] == 1.0 and head["supervised_q"] == 0.4
    assert head["supervised_eps"] == 0.01 and head["kitti_flow"] == "/x"
    assert head["kitti_flow_holdout"] == 5 and head["photometric_weight"] == 0.0


@pytest.mark.parametrize("argv", [
    ["--kitti-flow", "/x", "--kitti", "/y"],
    ["--supervised-weight", "1", "--warp-convention", "image"],             # no --kitti-flow
    ["--supervised-weight", "1", "--kitti-flow", "/x"],                     # reference convention
    ["--supervised-weight", "-1", "--kitti-flow", "/x", "--warp-convention", "image"],
    ["--kitti-flow-holdout", "5"],
    ["--kitti-flow-holdout", "1", "--kitti-flow", "/x", "--warp-convention", "image"],
])
def test_train_command_rejects(argv, capsys):
    from optical_flow_amd.train import check_supervised_args, main
    with pytest.raises(ValueError):
        check_supervised_args(_parse(argv))
    with pytest.raises(SystemExit) as e:                # main: a parser error, before any GPU work
        main(argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_train_command_rejects_augmentation_of_labelled_frames(capsys):
    from optical_flow_amd.train import main
    with pytest.raises(SystemExit) as e:
        main(["--kitti-flow", "/x", "--augment"])
    assert e.value.code == 2
    assert "ground truth" in capsys.readouterr().err


# ------------------------------------------------------------------ labelled reader ----
def test_split_kitti_flow():
    from optical_flow_amd.evaluate import split_kitti_flow
    frames = [("a%02d" % i, "b%02d" % i, "c%02d" % i) for i in range(11)]
    train, val = split_kitti_flow(list(reversed(frames)), 5)
    assert val == [frames[4], frames[9]]
    assert train == [f for i, f in enumerate(frames) if i not in (4, 9)]
    assert sorted(train + val) == frames
    for bad in (0, 1, -3, 2.5, True):
        with pytest.raises(ValueError):
            split_kitti_flow(frames, bad)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """Five tiny labelled frames of two native sizes in KITTI's layout."""
    root = str(tmp_path_factory.mktemp("kitti_flow_train"))
    tr = os.path.join(root, "training")
    for d in ("image_2", "flow_occ"):
        os.makedirs(os.path.join(tr, d))
    rng = np.random.default_rng(5)
    maps = []
    for k in range(5):
        h, w = ((9, 14), (7, 12))[k % 2]
        for rel in ("image_2/%06d_10.png", "image_2/%06d_11.png"):
            K.write_png(os.path.join(tr, rel % k), rng.integers(0, 256, (h, w, 3)).astype(np.uint8))
        gmap = R.make_gt(rng.uniform(-5, 5, (h, w, 2)), rng)
        K.write_png(os.path.join(tr, "flow_occ/%06d_10.png" % k), gmap)
        maps.append(gmap)
    return root, maps


def test_reader_seeded_order_and_host_batches(tree):
    from optical_flow_amd.data_reader import AugmentOpts
    from optical_flow_amd.evaluate import KittiFlowReader, list_kitti_flow
    root, maps = tree
    r = KittiFlowReader(root, 2, 16, 32, seed=3, nworkers=2)
    assert r.nbatches == 2 and len(r.frames) == 5
    o0, o1 = r.order(0), r.order(1)
    assert len(o0) == 4 and len(set(o0)) == 4 and set(o0) <= set(range(5))    # short batch dropped
    assert o0 == KittiFlowReader(list_kitti_flow(root), 2, 16, 32, seed=3).order(0)
    assert o0 == r.order(0) and (o0 != o1 or o0 != r.order(2))                # per-epoch shuffle
    assert any(KittiFlowReader(root, 2, 16, 32, seed=s).order(0) != o0 for s in (4, 5, 6))
    batches = list(r.host_batches(0))
    assert [i for _, _, idx in batches for i in idx] == o0
    for pairs, gmaps, idx in batches:
        assert len(pairs) == len(gmaps) == 2
        for (a, b), g, i in zip(pairs, gmaps, idx):
            np.testing.assert_array_equal(g, maps[i])                         # decoded ground truth
            assert a.shape == b.shape == maps[i].shape and a.dtype == np.uint8
    with pytest.raises(ValueError, match="augment"):
        KittiFlowReader(root, 2, 16, 32, augment=AugmentOpts())
    with pytest.raises(ValueError, match="batch"):
        KittiFlowReader(root, 6, 16, 32)


# ------------------------------------------------------------ the C entry's checks ----
@pytest.fixture(scope="module")
def lib():
    from optical_flow_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def test_sizing_functions(lib):
    # small footprints: four cells per workgroup; above 1024 pixels: one cell per workgroup
    assert lib.of_supervised_partials(3, 8, 16, 37, 67) == 3 * 32
    assert lib.of_supervised_partials(3, 1, 2, 37, 67) == 3 * 2
    assert lib.of_supervised_partials(2, 96, 320, 375, 1242) == 2 * 96 * 320 // 4
    assert lib.of_supervised_partials(2, 12, 40, 375, 1242) == 2 * 12 * 40
    assert lib.of_supervised_partials(0, 8, 16, 37, 67) == 0
    assert lib.of_supervised_workspace_bytes(3, 37, 67) == 256 + 3 * 4
    assert lib.of_supervised_workspace_bytes(2, 375, 1242) == 256 + 2 * 114 * 4


def _fwd(lib, **over):
    """of_supervised_fwd_multi with every argument valid except ``over``; the pointers are host
    buffers, which no call here ever reaches a launch with."""
    L = over.get("levels", 2)
    k = max(L, 1)
    buf = (C.c_float * 512)()
    base = C.addressof(buf)
    base += (-base) % 16
    ptrs = lambda: (C.c_void_p * k)(*[base] * k)
    descs = np.zeros(2, np.dtype([("offset", np.int64), ("h", np.int32), ("w", np.int32)]))
    descs[0], descs[1] = (256, 4, 5), (512, 3, 3)
    a = dict(flows=ptrs(), n=2, n_gt=2, fhs=(C.c_int * k)(*[3] * k), fws=(C.c_int * k)(*[4] * k),
             levels=L, raw=base, descs=descs, gt_bytes=1024, max_gh=4, max_gw=5, q=1.0, eps=0.01,
             coefs=(C.c_float * k)(*[1.0] * k), ws=base, ws_bytes=1024, dsdfs=ptrs(),
             partials=base)
    a.update(over)
    d = a["descs"]
    return lib.of_supervised_fwd_multi(
        a["flows"], a["n"], a["n_gt"], a["fhs"], a["fws"], a["levels"], a["raw"],
        d.ctypes.data_as(C.c_void_p) if d is not None else None, a["gt_bytes"], a["max_gh"],
        a["max_gw"], a["q"], a["eps"], a["coefs"], a["ws"], a["ws_bytes"], a["dsdfs"],
        a["partials"], None)


def _null_entry():
    p = (C.c_void_p * 2)()
    buf = (C.c_float * 8)()
    p[0] = C.addressof(buf) + (-C.addressof(buf)) % 8
    p._keep = buf
    return p                                   # entry 1 is NULL


def _descs(*rows):
    d = np.zeros(len(rows), np.dtype([("offset", np.int64), ("h", np.int32), ("w", np.int32)]))
    for i, r in enumerate(rows):
        d[i] = r
    return d


BAD = [("levels0", dict(levels=0)), ("levels9", dict(levels=9)), ("n0", dict(n=0)),
       ("n_gt0", dict(n_gt=0)), ("n_gt3", dict(n_gt=3)),
       ("h0", dict(fhs=(C.c_int * 2)(3, 0))), ("w0", dict(fws=(C.c_int * 2)(0, 4))),
       ("q0", dict(q=0.0)), ("q2.5", dict(q=2.5)), ("qnan", dict(q=float("nan"))),
       ("eps0", dict(eps=0.0)), ("eps-1", dict(eps=-1.0)),
       ("max_gh0", dict(max_gh=0)), ("max_gw0", dict(max_gw=0)),
       ("flows", dict(flows=None)), ("raw", dict(raw=None)), ("partials", dict(partials=None)),
       ("workspace", dict(ws=None)), ("workspace small", dict(ws_bytes=8)),
       ("flows[1]", dict(flows=_null_entry())), ("dsdfs[1]", dict(dsdfs=_null_entry())),
       ("desc size", dict(descs=_descs((256, 0, 5), (512, 3, 3)))),
       ("desc in header", dict(descs=_descs((0, 4, 5), (512, 3, 3)))),
       ("desc past end", dict(descs=_descs((256, 4, 5), (1020, 3, 3))))]


@pytest.mark.parametrize("name,over", BAD, ids=[b[0] for b in BAD])
def test_einval(lib, name, over):
    assert _fwd(lib, **over) == 1                      # OF_EINVAL, no exception, no launch
    assert b"of_supervised_fwd_multi" in lib.of_last_error()


def test_misaligned_pointers_are_einval(lib):
    buf = (C.c_float * 512)()
    base = C.addressof(buf)
    base += (-base) % 16
    assert _fwd(lib, raw=base + 8) == 1 and b"16-byte" in lib.of_last_error()
    assert _fwd(lib, ws=base + 4) == 1
    odd = (C.c_void_p * 2)(base, base + 4)
    assert _fwd(lib, flows=odd) == 1 and b"8-byte" in lib.of_last_error()
