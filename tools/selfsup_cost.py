"""Cost of augmentation self-supervision in the eager train step (GPU; DESIGN.md
"Self-supervision").

python tools/selfsup_cost.py [--rounds 30] [--reps 5] [--out selfsup_cost.json]

Trainer.train_step at the bench's headline shape (384 x 512, B = 8, fp32, bench.py's initial
weights and batch), image warp convention, in two arms: the plain step, and the self-supervised
step (LossLayer selfsup_weight 0.3, transform zoom 1-1.3 and flip 0.5: a teacher pass, the
augmentation, the flow transform and the distill term on top of the plain step).  The
self-supervised step is not captured as a graph, so eager is compared with eager.  One process;
each arm has a net, an optimizer and a trainer of its own, and the arms are alternated window by
window (so they see the same neighbours on the machine); a window is ``--reps`` steps between
two device events, after ``--warmup`` untimed windows per arm.  Prints one JSON line: per arm
the median, quartiles and extremes of the step time in ms, the self-supervised arm over the
plain one, and the bytes that each of the three new kernels must move at this shape with the
least time that the HBM peak allows for them.

Kernel times come from a kernel trace of a short run, a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o selfsup -- \
        python tools/selfsup_cost.py --rounds 3
``--kernel-stats FILE`` reads that run's kernel_stats csv and sets each new kernel's average
time against its least time.
"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12           # bytes/s: the MI355X's HBM3E spec peak
HBM_ACHIEVABLE = 6.3e12     # what a float4 copy reaches on it


def kernel_bytes(B, H, W):
    """Bytes each new kernel must move at this shape (fp32; compulsory traffic: each input
    element read once, each output element written once; the 64-byte records are noise)."""
    fh, fw = H // 2, W // 2
    cells = B * fh * fw
    return {
        # batch in, batch out
        "augment_batch_kernel": 2 * B * H * W * 6 * 4,
        # teacher and mask in, target and weight out
        "flow_transform_kernel": cells * (2 + 1 + 2 + 1) * 4,
        # student, target and weight in, plane out
        "flow_distill_kernel": cells * (2 + 2 + 1 + 2) * 4,
    }


def read_kernel_stats(path):
    """{kernel: (calls, average ns)} of the new kernels from rocprofv3's kernel_stats csv."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            for k in ("augment_batch_kernel", "flow_transform_kernel", "flow_distill_kernel"):
                if k in name:
                    calls = int(row.get("Calls") or row.get("Count") or 0)
                    avg = float(row.get("AverageNs") or row.get("Average") or 0.0)
                    prev = out.get(k, (0, 0.0))
                    tot = prev[0] + calls
                    out[k] = (tot, (prev[0] * prev[1] + calls * avg) / max(tot, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30, help="timed windows per arm")
    ap.add_argument("--reps", type=int, default=5, help="steps per window")
    ap.add_argument("--warmup", type=int, default=3, help="untimed windows per arm")
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--occlusion", default="none", choices=("none", "border", "fb", "range"))
    ap.add_argument("--kernel-stats", default=None, metavar="FILE",
                    help="a rocprofv3 kernel_stats csv: only set the new kernels' times "
                         "against their bytes, no GPU run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    H, W, B = args.height, args.width, args.batch
    nbytes = kernel_bytes(B, H, W)
    floors = {k: {"bytes": v, "least_us_at_peak": round(v / HBM_PEAK * 1e6, 3),
                  "least_us_achievable": round(v / HBM_ACHIEVABLE * 1e6, 3)}
              for k, v in nbytes.items()}
    if args.kernel_stats:
        for k, (calls, avg_ns) in read_kernel_stats(args.kernel_stats).items():
            floors[k].update(calls=calls, average_us=round(avg_ns / 1e3, 3),
                             share_of_peak=round(nbytes[k] / HBM_PEAK / (avg_ns * 1e-9), 4)
                             if avg_ns > 0 else None)
        print(json.dumps({"size": [B, H, W], "kernels": floors}), flush=True)
        return
    if not torch.cuda.is_available():
        sys.exit("selfsup_cost.py measures on the GPU; none is visible")
    from optical_flow_amd import _lib
    from optical_flow_amd.data import synthetic_batch
    from optical_flow_amd.data_reader import AugmentOpts
    from optical_flow_amd.loss import LossLayer
    from optical_flow_amd.model import FlowNet
    from optical_flow_amd.params import flow_net_spec, init_params
    from optical_flow_amd.train import KerasAdam, Trainer
    _lib.load()
    batch = torch.from_numpy(synthetic_batch(B, H, W, seed=1234)).cuda()
    arms = [("plain", 0.0), ("selfsup", 0.3)]
    steps = []
    for _, w in arms:
        net = FlowNet(H, W, values=init_params(flow_net_spec(levels=4), 0),
                      warp_convention="image")
        layer = LossLayer(warp_convention="image", occlusion=args.occlusion, selfsup_weight=w)
        opts = AugmentOpts(zoom=(1.0, 1.3), hflip_prob=0.5) if w else None
        trainer = Trainer(net, KerasAdam(net.store), layer, data_parallel=False, selfsup=opts)
        steps.append(lambda t=trainer: t.train_step(batch))
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
    rec = {"size": [B, H, W], "rounds": args.rounds, "reps": args.reps, "step": "eager",
           "occlusion": args.occlusion, "arms": {}, "kernels": floors}
    for (name, _), t in zip(arms, times):
        q = np.percentile(t, [25, 50, 75])
        rec["arms"][name] = {"median_ms": round(float(q[1]), 4), "q25_ms": round(float(q[0]), 4),
                             "q75_ms": round(float(q[2]), 4), "min_ms": round(float(min(t)), 4),
                             "max_ms": round(float(max(t)), 4)}
    base = rec["arms"]["plain"]["median_ms"]
    own = rec["arms"]["selfsup"]
    own["over_plain_ms"] = round(own["median_ms"] - base, 4)
    own["over_plain_ratio"] = round(own["median_ms"] / base, 4)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
