"""Cost of labelled augmentation (GPU; DESIGN.md §3 "Labelled augmentation").

python tools/gt_augment_cost.py [--rounds 30] [--reps 5] [--out gt_augment_cost.json]

Two measurements, one process, one JSON line.

kernel  of_gt_augment on eight 375 x 1242 maps (30 % of the pixels valid, records drawn from the
        train command's preset) between two device events, ``--kernel-reps`` launches per window,
        beside of_flow_eval on the same batch (a 192 x 640 flow) timed the same way in the same
        windows, and beside the bytes the kernel must move (6 read + 6 written per pixel) over the
        HBM peak.
step    the fine-tuning step at 384 x 512, B = 8 on labelled frames of 375 x 1242 held in host
        memory (no PNG decode: the reader's decode threads run ahead of the GPU), in two arms
        alternated window by window: ``plain`` is the un-augmented labelled batch as
        KittiFlowReader makes it (upload, of_preprocess_pairs, ground-truth upload) and one
        supervised train_step; ``augmented`` draws the records, runs of_augment_pairs and
        of_gt_augment in their place, then the same train_step.  Each arm has a net, an optimizer
        and a trainer of its own.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12           # bytes/s: the MI355X's HBM3E spec peak
HBM_ACHIEVABLE = 6.3e12     # what a float4 copy reaches on it
GH, GW = 375, 1242


def _stats(t):
    q = np.percentile(t, [25, 50, 75])
    return {"median": round(float(q[1]), 4), "q25": round(float(q[0]), 4),
            "q75": round(float(q[2]), 4), "min": round(float(min(t)), 4),
            "max": round(float(max(t)), 4)}


def _window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def make_maps(n, rng):
    maps = []
    for _ in range(n):
        rgb = np.zeros((GH, GW, 3), np.uint16)
        rgb[..., :2] = np.rint(rng.uniform(-40, 40, (GH, GW, 2)) * 64 + 32768).astype(np.uint16)
        rgb[..., 2] = rng.uniform(size=(GH, GW)) < 0.3
        maps.append(rgb)
    return maps


def kernel_times(args, preset):
    from optical_flow_amd import ops
    from optical_flow_amd._lib import call, lib
    from optical_flow_amd.data_reader import sample_augment
    from optical_flow_amd.gt_raw import pack_gt_raw
    rng = np.random.default_rng(0)
    n = 8
    raw, descs = pack_gt_raw(make_maps(n, rng))
    src = torch.from_numpy(raw).cuda()
    dst = torch.empty_like(src)
    rec = ops._records_dev(sample_augment(preset, n, 384, 512, 0, 0), n, src.device)
    flow = torch.from_numpy(rng.uniform(-3, 3, (n, 192, 640, 2)).astype(np.float32)).cuda()
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dp = descs.ctypes.data_as(C.c_void_p)

    def augment():
        call("of_gt_augment", C.c_void_p(src.data_ptr()), dp, src.numel(), n, 384, 512,
             C.c_void_p(rec.data_ptr()), C.c_void_p(dst.data_ptr()), stream())

    npart = lib().of_flow_eval_partials(n, GH, GW)
    partials = torch.empty(3 * npart, dtype=torch.float64, device="cuda")
    res = torch.empty((n, 3), dtype=torch.int64, device="cuda")

    def evaluate():                     # evaluate.flow_metrics' call, buffers made once
        call("of_flow_eval", C.c_void_p(flow.data_ptr()), n, 192, 640, C.c_void_p(src.data_ptr()),
             dp, src.numel(), C.c_void_p(partials.data_ptr()), npart, C.c_void_p(res.data_ptr()),
             stream())

    t = {"of_gt_augment": [], "of_flow_eval": []}
    for r in range(args.warmup + args.rounds):
        for name, fn in (("of_gt_augment", augment), ("of_flow_eval", evaluate)):
            us = 1e3 * _window(fn, args.kernel_reps)
            if r >= args.warmup:
                t[name].append(us)
    pixels = n * GH * GW
    nbytes = 12 * pixels
    out = {"maps": [n, GH, GW], "reps_per_window": args.kernel_reps,
           "of_gt_augment_us": _stats(t["of_gt_augment"]),
           "of_flow_eval_us": _stats(t["of_flow_eval"]),
           "bytes": nbytes, "least_us_at_peak": round(nbytes / HBM_PEAK * 1e6, 3),
           "least_us_achievable": round(nbytes / HBM_ACHIEVABLE * 1e6, 3)}
    med = out["of_gt_augment_us"]["median"]
    out["bytes_per_s"] = round(nbytes / (med * 1e-6), 0)
    out["share_of_peak"] = round(nbytes / HBM_PEAK / (med * 1e-6), 4)
    return out


def step_times(args, preset):
    from optical_flow_amd import ops
    from optical_flow_amd._lib import call
    from optical_flow_amd.data_reader import _pack_raw, sample_augment
    from optical_flow_amd.gt_raw import _upload, pack_gt_raw
    from optical_flow_amd.loss import LossLayer
    from optical_flow_amd.model import FlowNet
    from optical_flow_amd.params import flow_net_spec, init_params
    from optical_flow_amd.train import KerasAdam, Trainer
    H, W, B = args.height, args.width, args.batch
    rng = np.random.default_rng(1)
    pairs = [(rng.integers(0, 256, (GH, GW, 3)).astype(np.uint8),
              rng.integers(0, 256, (GH, GW, 3)).astype(np.uint8)) for _ in range(B)]
    frames = _pack_raw(pairs)
    raw, descs = pack_gt_raw(make_maps(B, rng))
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    count = [0]

    def labelled_batch(augment):
        dev = _upload(frames)
        batch = torch.empty((B, H, W, 6), device="cuda")
        if not augment:
            call("of_preprocess_pairs", C.c_void_p(dev.data_ptr()), B, H, W,
                 C.c_void_p(batch.data_ptr()), stream())
            return batch, (_upload(raw), descs)
        count[0] += 1
        rec = _upload(sample_augment(preset, B, H, W, 0, count[0]).view(np.uint8))
        call("of_augment_pairs", C.c_void_p(dev.data_ptr()), B, H, W, C.c_void_p(rec.data_ptr()),
             C.c_void_p(batch.data_ptr()), stream())
        return batch, ops.augment_gt((_upload(raw), descs), rec, (H, W))

    arms = ["plain", "augmented"]
    steps = []
    for name in arms:
        net = FlowNet(H, W, values=init_params(flow_net_spec(levels=4), 0),
                      warp_convention="image")
        layer = LossLayer(warp_convention="image", photometric_weight=0.0, supervised_weight=1.0)
        trainer = Trainer(net, KerasAdam(net.store), layer, data_parallel=False)

        def step(t=trainer, aug=name == "augmented"):
            batch, gt = labelled_batch(aug)
            t.train_step(batch, gt=gt)
        steps.append(step)
    times = [[] for _ in arms]
    for r in range(args.warmup + args.rounds):
        for k, step in enumerate(steps):
            ms = _window(step, args.reps)
            if r >= args.warmup:
                times[k].append(ms)
    out = {"size": [B, H, W], "frames": [GH, GW], "reps_per_window": args.reps,
           "arms_ms": {a: _stats(t) for a, t in zip(arms, times)}}
    base, own = out["arms_ms"]["plain"]["median"], out["arms_ms"]["augmented"]["median"]
    out["augmented_over_plain_ms"] = round(own - base, 4)
    out["augmented_over_plain_ratio"] = round(own / base, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30, help="timed windows per arm")
    ap.add_argument("--reps", type=int, default=5, help="steps per window")
    ap.add_argument("--kernel-reps", type=int, default=50, help="kernel launches per window")
    ap.add_argument("--warmup", type=int, default=3, help="untimed windows per arm")
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--skip-step", action="store_true", help="the kernel times only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gt_augment_cost.py measures on the GPU; none is visible")
    from optical_flow_amd import _lib
    from optical_flow_amd.data_reader import AugmentOpts
    from optical_flow_amd.train import AUGMENT_PRESET
    _lib.load()
    preset = AugmentOpts(**AUGMENT_PRESET)
    rec = {"kernel": kernel_times(args, preset)}
    if not args.skip_step:
        rec["step"] = step_times(args, preset)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
