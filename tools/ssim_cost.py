"""Cost of the SSIM data term in the graphed train step (GPU; DESIGN.md "SSIM term").

python tools/ssim_cost.py [--rounds 30] [--reps 5] [--out ssim_cost.json]

The captured step (Trainer.graphed) at the bench's headline shape (384 x 512, B = 8, fp32,
bench.py's initial weights and batch) in two arms that differ only in LossLayer's
``ssim_weight``: 0 against 0.85, both with the photometric term at 0.15.  One process; each arm
has a net, an optimizer and a captured step of its own, and the arms are alternated window by
window (so they see the same neighbours on the machine); a window is ``--reps`` replays between
two device events, after ``--warmup`` untimed windows per arm.  Prints one JSON line: per arm
the median, quartiles and minimum of the step time in ms and the SSIM arm over the other of the
same call.

Kernel times come from a kernel trace of a short eager run, a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ssim -- \
        python tools/ssim_cost.py --rounds 3 --eager --census
(--eager times Trainer.train_step itself, whose kernels a trace names one by one; --census adds
two arms with the census term at radius 1 and 3 in place of SSIM, so that the same trace holds
census_fwd_multi<1> and <3>, the yardsticks of ssim_fwd_multi.)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, LossLayer keywords beside photometric_weight = 0.15)
ARMS = [("ssim0", dict()), ("ssim0.85", dict(ssim_weight=0.85))]
CENSUS_ARMS = [("census0.85_r1", dict(census_weight=0.85, census_radius=1)),
               ("census0.85_r3", dict(census_weight=0.85, census_radius=3))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30, help="timed windows per arm")
    ap.add_argument("--reps", type=int, default=5, help="steps per window")
    ap.add_argument("--warmup", type=int, default=3, help="untimed windows per arm")
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--eager", action="store_true", help="time train_step, not the captured step")
    ap.add_argument("--census", action="store_true",
                    help="two more arms with the census term (radius 1 and 3) in place of SSIM")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ssim_cost.py measures on the GPU; none is visible")
    from optical_flow_amd import _lib
    from optical_flow_amd.data import synthetic_batch
    from optical_flow_amd.loss import LossLayer
    from optical_flow_amd.model import FlowNet
    from optical_flow_amd.params import flow_net_spec, init_params
    from optical_flow_amd.train import KerasAdam, Trainer
    _lib.load()
    H, W, B = args.height, args.width, args.batch
    batch = torch.from_numpy(synthetic_batch(B, H, W, seed=1234)).cuda()
    arms = ARMS + (CENSUS_ARMS if args.census else [])
    steps = []
    for _, kw in arms:
        net = FlowNet(H, W, values=init_params(flow_net_spec(levels=4), 0))
        trainer = Trainer(net, KerasAdam(net.store), LossLayer(photometric_weight=0.15, **kw))
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
           "step": "eager" if args.eager else "graphed", "arms": {}}
    for (name, _), t in zip(arms, times):
        q = np.percentile(t, [25, 50, 75])
        rec["arms"][name] = {"median_ms": round(float(q[1]), 4), "q25_ms": round(float(q[0]), 4),
                             "q75_ms": round(float(q[2]), 4), "min_ms": round(float(min(t)), 4),
                             "max_ms": round(float(max(t)), 4)}
    base = rec["arms"][arms[0][0]]["median_ms"]
    for name, _ in arms[1:]:
        rec["arms"][name]["over_ssim0_ms"] = round(rec["arms"][name]["median_ms"] - base, 4)
        rec["arms"][name]["over_ssim0_ratio"] = round(rec["arms"][name]["median_ms"] / base, 4)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
