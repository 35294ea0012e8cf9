"""Cost of the occlusion masks in the graphed train step (GPU; DESIGN.md "Occlusion masks").

python tools/occlusion_step_time.py [--rounds 30] [--reps 5] [--out occlusion_step.json]

The captured step (Trainer.graphed) at the bench's headline shape (384 x 512, B = 8, fp32,
bench.py's initial weights and batch) in the image convention with census + smoothness, in
four arms that differ only in LossLayer's ``occlusion``: "none", "border", "fb" and "range"
(the last two run the net on 2B images; --arms picks a subset, "none" always among them).
One process; each arm has a net, an optimizer and a captured step of its own, and the arms
are alternated window by window (so they see the same neighbours on the machine); a window is ``--reps`` replays between two device events, after ``--warmup``
untimed windows per arm.  Prints one JSON line: per arm the median, quartiles and minimum of
the step time in ms, "none"'s own spread, the other arms over "none" of the same call, and
"range" over "fb" when both ran.

Kernel times (occ_mask_multi, occ_range_zero / _splat / _finish, photo_l1_*_multi with
weights, census_fwd_multi with weights) come from a kernel trace of a short run of this script,
a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o occ -- \
        python tools/occlusion_step_time.py --rounds 3 --eager --photometric-weight 1
(--eager times Trainer.train_step itself, whose kernels a trace names one by one;
--photometric-weight 1 adds the photometric term, so the trace holds its weighted kernels too.)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = ["none", "border", "fb", "range"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30, help="timed windows per arm")
    ap.add_argument("--reps", type=int, default=5, help="steps per window")
    ap.add_argument("--warmup", type=int, default=3, help="untimed windows per arm")
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--eager", action="store_true", help="time train_step, not the captured step")
    ap.add_argument("--photometric-weight", type=float, default=0.0,
                    help="weight of the photometric term beside census + smoothness (a trace "
                         "with 1 shows the weighted photometric kernels too)")
    ap.add_argument("--arms", default=",".join(ARMS),
                    help="comma-separated subset of %s; \"none\" is always run" % ARMS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    arms = [a for a in ARMS if a == "none" or a in args.arms.split(",")]
    if set(args.arms.split(",")) - set(ARMS):
        ap.error("--arms takes %s" % ARMS)
    if not torch.cuda.is_available():
        sys.exit("occlusion_step_time.py measures on the GPU; none is visible")
    from optical_flow_amd import _lib
    from optical_flow_amd.data import synthetic_batch
    from optical_flow_amd.loss import LossLayer
    from optical_flow_amd.model import FlowNet
    from optical_flow_amd.params import flow_net_spec, init_params
    from optical_flow_amd.train import KerasAdam, Trainer
    _lib.load()
    H, W, B = args.height, args.width, args.batch
    batch = torch.from_numpy(synthetic_batch(B, H, W, seed=1234)).cuda()
    steps = []
    for mode in arms:
        net = FlowNet(H, W, values=init_params(flow_net_spec(levels=4), 0),
                      warp_convention="image")
        layer = LossLayer(0.2, 10, census_weight=1.0, photometric_weight=args.photometric_weight,
                          warp_convention="image", occlusion=mode)
        trainer = Trainer(net, KerasAdam(net.store), layer)
        if args.eager:
            steps.append(lambda t=trainer: t.train_step(batch))
        else:
            g = trainer.graphed(batch.clone(), warmup=2)
            steps.append(lambda g=g: g())
    times = [[] for _ in arms]
    for r in range(args.warmup + args.rounds):
        for k, step in enumerate(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                step()
            e1.record()
            e1.synchronize()
            if r >= args.warmup:
                times[k].append(e0.elapsed_time(e1) / args.reps)
    rec = {"size": [B, H, W], "rounds": args.rounds, "reps": args.reps,
           "photometric_weight": args.photometric_weight,
           "step": "eager" if args.eager else "graphed", "arms": {}}
    for name, t in zip(arms, times):
        q = np.percentile(t, [25, 50, 75])
        rec["arms"][name] = {"median_ms": round(float(q[1]), 4), "q25_ms": round(float(q[0]), 4),
                             "q75_ms": round(float(q[2]), 4), "min_ms": round(float(min(t)), 4),
                             "max_ms": round(float(max(t)), 4)}
    base = rec["arms"]["none"]["median_ms"]
    rec["none_iqr_ms"] = round(rec["arms"]["none"]["q75_ms"] - rec["arms"]["none"]["q25_ms"], 4)
    for name in arms[1:]:
        rec["arms"][name]["over_none_ms"] = round(rec["arms"][name]["median_ms"] - base, 4)
        rec["arms"][name]["over_none_ratio"] = round(rec["arms"][name]["median_ms"] / base, 4)
    if "fb" in arms and "range" in arms:
        rec["range_over_fb_ms"] = round(rec["arms"]["range"]["median_ms"] -
                                        rec["arms"]["fb"]["median_ms"], 4)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
