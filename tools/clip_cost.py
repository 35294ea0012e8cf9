"""Cost of global-norm clipping and the non-finite guard (GPU; DESIGN.md "Gradient clipping and
the non-finite guard").

python tools/clip_cost.py [--launches 200] [--rounds 20] [--warmup 3] [--out clip_cost.json]

Two measurements, one JSON line:

kernels: at the flow net's arena (4.94 M floats) with standard-normal gradients, the launches of
    of_grad_sumsq, of_adam_keras_dev (sched + update) and of_adam_keras_dev_clip (sched + update)
    back to back on one stream, ``--launches`` of one kind between a device event pair, five
    such batches per kind, the kinds interleaved; per kind the median and minimum microseconds
    per call and the bytes it moves over that time (sumsq reads the arena once, 19.7 MB; the
    Adam updates read four arenas and write three, 138 MB).  Back to back the arenas stay in
    the 256 MiB Infinity Cache, as the gradient arena does between the backward, the norm and
    the update of a real step.  lr is 0 in these launches.

step: Trainer.train_step at the bench size (384 x 512, B = 8, fp32, bench.py's initial weights and
    batch) in arms that differ only in the optimizer -- plain KerasAdam, track_grad_norm,
    global_clipnorm (``--clip-norm``), global_clipnorm + skip_nonfinite -- over one net, each
    arm with moments of its own, alternated step by step, each step timed by a device event
    pair after ``--warmup`` steps per arm: per arm the median, quartiles and minimum in ms and
    the median over the plain arm of the same call.
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


def _stats(t):
    q = np.percentile(t, [25, 50, 75])
    return {"median": round(float(q[1]), 4), "q25": round(float(q[0]), 4),
            "q75": round(float(q[2]), 4), "min": round(float(min(t)), 4)}


def kernels(args):
    from optical_flow_amd import _lib, ops
    from optical_flow_amd._lib import call
    lib = _lib.lib()
    n = args.numel
    P = lib.of_grad_sumsq_partials(n)
    g = torch.randn(n, device="cuda")
    p, m, v = (torch.zeros(n, device="cuda") for _ in range(3))
    sched = torch.zeros(2, device="cuda")
    it = torch.zeros(1, dtype=torch.int32, device="cuda")
    part = torch.zeros(P, dtype=torch.float64, device="cuda")
    state = torch.zeros(lib.of_adam_clip_state_bytes() // 8, dtype=torch.float64, device="cuda")
    vp = lambda t: C.c_void_p(t.data_ptr())
    st = ops._stream()

    def sumsq():
        call("of_grad_sumsq", vp(g), n, vp(part), st)

    def adam():
        call("of_adam_keras_dev", vp(p), vp(g), vp(m), vp(v), n, vp(sched), vp(it), 0.9, 0.999,
             1e-7, 1.0, st)

    def adam_clip():
        call("of_adam_keras_dev_clip", vp(p), vp(g), vp(m), vp(v), n, vp(sched), vp(it), 0.9,
             0.999, 1e-7, 1.0, vp(part), P, 1.0, 1, vp(state), st)

    def both():
        sumsq()
        adam_clip()

    kinds = [("grad_sumsq", sumsq, 4 * n), ("adam_keras_dev", adam, 28 * n),
             ("adam_keras_dev_clip", adam_clip, 28 * n), ("sumsq_plus_adam_clip", both, 32 * n)]
    times = {k: [] for k, _, _ in kinds}
    for rep in range(6):                         # the first batch of each kind is warm-up
        for name, fn, _ in kinds:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                fn()
            e1.record()
            e1.synchronize()
            if rep:
                times[name].append(1e3 * e0.elapsed_time(e1) / args.launches)
    out = {"numel": n, "partials": P, "launches": args.launches}
    for name, _, nbytes in kinds:
        s = _stats(times[name])
        out[name] = {"us_median": s["median"], "us_min": s["min"], "bytes": nbytes,
                     "tb_per_s_at_median": round(nbytes / s["median"] * 1e-6, 3)}
    return out


def step(args):
    from optical_flow_amd.data import synthetic_batch
    from optical_flow_amd.loss import LossLayer
    from optical_flow_amd.model import FlowNet
    from optical_flow_amd.params import flow_net_spec, init_params
    from optical_flow_amd.train import KerasAdam, Trainer
    H, W, B = args.height, args.width, args.batch
    net = FlowNet(H, W, values=init_params(flow_net_spec(levels=4), 0))
    arms = [("plain", {}), ("track", dict(track_grad_norm=True)),
            ("clip", dict(global_clipnorm=args.clip_norm)),
            ("clip_guard", dict(global_clipnorm=args.clip_norm, skip_nonfinite=True))]
    opts = [KerasAdam(net.store, **kw) for _, kw in arms]
    trainer = Trainer(net, opts[0], LossLayer())
    batch = torch.from_numpy(synthetic_batch(B, H, W, seed=1234)).cuda()
    times = [[] for _ in arms]
    k = 0
    for r in range(args.warmup + args.rounds):
        for a, opt in enumerate(opts):
            trainer.optimizer = opt
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            trainer.train_step(batch, k)
            e1.record()
            e1.synchronize()
            if r >= args.warmup:
                times[a].append(e0.elapsed_time(e1))
            k += 1
    out = {"size": [B, H, W], "rounds": args.rounds, "clip_norm": args.clip_norm, "arms": {}}
    for (name, _), t in zip(arms, times):
        s = _stats(t)
        out["arms"][name] = {key + "_ms": val for key, val in s.items()}
    base = out["arms"]["plain"]["median_ms"]
    for name, _ in arms[1:]:
        a = out["arms"][name]
        a["over_plain_ms"] = round(a["median_ms"] - base, 4)
        a["over_plain_pct"] = round(100.0 * (a["median_ms"] / base - 1.0), 2)
    out["last_grad_norm"] = float(opts[2].last_grad_norm)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--numel", type=int, default=4937219, help="arena size of the kernel timing")
    ap.add_argument("--launches", type=int, default=200, help="launches per event pair")
    ap.add_argument("--rounds", type=int, default=20, help="timed steps per arm")
    ap.add_argument("--warmup", type=int, default=3, help="untimed steps per arm")
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--clip-norm", type=float, default=1.0)
    ap.add_argument("--no-step", action="store_true", help="kernel timing only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("clip_cost.py measures on the GPU; none is visible")
    from optical_flow_amd import _lib
    _lib.load()
    rec = {"kernels": kernels(args)}
    if not args.no_step:
        rec["step"] = step(args)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
