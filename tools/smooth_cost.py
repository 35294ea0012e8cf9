"""Cost of the flow smoothness term in a train step (GPU; DESIGN.md "Flow smoothness term").

python tools/smooth_cost.py [--rounds 20] [--warmup 3] [--out smooth_cost.json]

Trainer.train_step at the bench size (384 x 512, B = 8, fp32, bench.py's initial weights and
batch) in five arms that differ only in the loss layer: weight 0 (the reference loss), weight
0.2 with edge_alpha 0 and with edge_alpha 10, and the same two with the second-order term
(smoothness_order=2).  One net and one optimizer; the arms are
alternated step by step (so they see the same drifting state and the same neighbours on the
machine), each step timed by a device event pair, after ``--warmup`` steps per arm.  Prints one
JSON line: per arm the median, quartiles and minimum of the step time in ms.

Kernel times (of_photo_l1_*_multi against of_flow_smooth_*_multi and of_flow_smooth2_*_multi)
come from a kernel trace of a
short run of this script, a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o cost -- \
        python tools/smooth_cost.py --rounds 5
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, smoothness_weight, edge_alpha, smoothness_order)
ARMS = [("weight0", 0.0, 0.0, 1), ("weight0.2_alpha0", 0.2, 0.0, 1),
        ("weight0.2_alpha10", 0.2, 10.0, 1), ("order2_weight0.2_alpha0", 0.2, 0.0, 2),
        ("order2_weight0.2_alpha10", 0.2, 10.0, 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20, help="timed steps per arm")
    ap.add_argument("--warmup", type=int, default=3, help="untimed steps per arm")
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("smooth_cost.py measures on the GPU; none is visible")
    from optical_flow_amd import _lib
    from optical_flow_amd.data import synthetic_batch
    from optical_flow_amd.loss import LossLayer
    from optical_flow_amd.model import FlowNet
    from optical_flow_amd.params import flow_net_spec, init_params
    from optical_flow_amd.train import KerasAdam, Trainer
    _lib.load()
    H, W, B = args.height, args.width, args.batch
    net = FlowNet(H, W, values=init_params(flow_net_spec(levels=4), 0))
    trainer = Trainer(net, KerasAdam(net.store), LossLayer())
    batch = torch.from_numpy(synthetic_batch(B, H, W, seed=1234)).cuda()
    layers = [LossLayer(w, a, smoothness_order=o) for _, w, a, o in ARMS]
    times = [[] for _ in ARMS]
    step = 0
    for r in range(args.warmup + args.rounds):
        for k, layer in enumerate(layers):
            trainer.loss_layer = layer
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            trainer.train_step(batch, step)
            e1.record()
            e1.synchronize()
            if r >= args.warmup:
                times[k].append(e0.elapsed_time(e1))
            step += 1
    rec = {"size": [B, H, W], "rounds": args.rounds, "arms": {}}
    for (name, w, a, o), t in zip(ARMS, times):
        q = np.percentile(t, [25, 50, 75])
        rec["arms"][name] = {"median_ms": round(float(q[1]), 4), "q25_ms": round(float(q[0]), 4),
                             "q75_ms": round(float(q[2]), 4), "min_ms": round(float(min(t)), 4)}
    base = rec["arms"][ARMS[0][0]]["median_ms"]
    for name, _, _, _ in ARMS[1:]:
        rec["arms"][name]["over_weight0_pct"] = round(
            100.0 * (rec["arms"][name]["median_ms"] / base - 1.0), 2)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
