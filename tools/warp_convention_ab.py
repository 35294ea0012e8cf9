#!/usr/bin/env python
"""The two warp conventions side by side, in ONE process on one box (GPU):

python tools/warp_convention_ab.py [--out profiles/warp_convention_ab.txt]

1. step:   the whole fp32 training step (Trainer.train_step, eager) at 384x512, batch 8, with
           warp_convention "reference" and "image", the two forms alternating round by round
           (reference, image, reference, image, ...) as tools/augment_step_ab.py alternates
           its runs; the same weights and the same batch in both.
2. kernel: per flow-module level, the deterministic warp backward (of_warp_bwd_det_cv) in both
           conventions, alternating, on random flows of std --mode-a-scales (mode A: R <= 8,
           drawn as tools/flow_bench.py draws them) and of std --fixed-scale (the fixed-point
           path); the path that served is read from the workspace header.
3. learn:  --learn-steps steps on one fixed synthetic_batch in each convention, logging the
           loss and the endpoint error of the finest flow (H/2) against the pair's known shift:
           data.synthetic_batch makes image 2[y, x] = image 1[y + dy, x + dx], so the true
           flow in image coordinates is (-dx, -dy) / 2 there.  Whatever happens is recorded;
           fp32 trajectories make excursions (README) and nothing is required of the outcome.

The yardstick of every comparison is the reference convention IN THE SAME CALL, and its margin
is the spread (max - min) of the reference convention's own rounds.  Times: host clock around
steps that end in a device synchronise (step), device events around `reps` launches (kernel).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from optical_flow_amd import _lib, ops  # noqa: E402
from optical_flow_amd._lib import call  # noqa: E402

FORMS = ("reference", "image")
# level, h, w, c at 384x512 (tools/flow_bench.py's LEVELS with a warp)
LEVELS = [(3, 192, 256, 64), (2, 96, 128, 64), (1, 48, 64, 128)]


def spread(v):
    return max(v) - min(v)


def make_trainer(h, w, convention, seed, lr):
    from optical_flow_amd.loss import LossLayer
    from optical_flow_amd.model import build_flow_net
    from optical_flow_amd.train import KerasAdam, Trainer
    net = build_flow_net(h, w, seed=seed, warp_convention=convention)
    return Trainer(net, KerasAdam(net.store, learning_rate=lr),
                   LossLayer(warp_convention=convention))


def step_ab(args, emit):
    from optical_flow_amd.data import synthetic_batch
    h, w, b = args.height, args.width, args.batch
    batch = torch.from_numpy(synthetic_batch(b, h, w, seed=1234)).cuda()
    tr = {f: make_trainer(h, w, f, args.seed, 1e-4) for f in FORMS}
    for f in FORMS:
        for k in range(args.warmup):
            tr[f].train_step(batch, k)
    torch.cuda.synchronize()
    ms = {f: [] for f in FORMS}
    for rnd in range(args.rounds):
        for f in FORMS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(args.steps):
                tr[f].train_step(batch, k)
            torch.cuda.synchronize()
            ms[f].append((time.perf_counter() - t0) / args.steps * 1e3)
    res = {"shape": [b, h, w], "steps_per_round": args.steps, "rounds": args.rounds,
           "ms": {f: [round(v, 3) for v in ms[f]] for f in FORMS},
           "median_ms": {f: round(float(np.median(ms[f])), 3) for f in FORMS},
           "reference_spread_ms": round(spread(ms["reference"]), 3)}
    emit("step %dx%dx%d fp32, ms per step by round: reference %s image %s" %
         (b, h, w, res["ms"]["reference"], res["ms"]["image"]))
    emit("step median: reference %.3f ms, image %.3f ms (%+.3f); reference spread %.3f ms" %
         (res["median_ms"]["reference"], res["median_ms"]["image"],
          res["median_ms"]["image"] - res["median_ms"]["reference"], res["reference_spread_ms"]))
    return res


def det_path(ws, hoff, npix):
    hdr = ws[hoff // 4: hoff // 4 + 64 * 129].cpu()
    rr = max(int(hdr[64 * (33 + k)]) for k in range(32))
    found = sum(int(hdr[64 * (1 + k)]) for k in range(32))
    rmax = 8
    return ("A" if rr <= rmax else "B" if found == 4 * npix else "fixed"), rr


def kernel_ab(args, emit):
    lib = _lib.lib()
    n = args.batch
    P = ops._ptr
    st = ops._stream()
    out = []
    scales = [(s, "A") for s in args.mode_a_scales] + [(args.fixed_scale, "fixed")]
    for lvl, h, w, c in LEVELS:
        g = torch.Generator(device="cuda").manual_seed(100 + lvl)
        f2 = torch.randn(n, h, w, c, device="cuda", generator=g)
        dout = torch.randn(n, h, w, c, device="cuda", generator=g)
        unit = torch.randn(n, h, w, 2, device="cuda", generator=g)
        dinp = torch.empty_like(f2)
        dfl = torch.empty(n, h, w, 2, device="cuda")
        wsb = lib.of_warp_bwd_det_workspace(n, h, w, c)
        hoff = lib.of_warp_bwd_det_header(n, h, w, c)
        ws = torch.zeros(wsb // 4 + 4, dtype=torch.int32, device="cuda")
        for scale, want in scales:
            fl = (unit * scale).contiguous()
            if want == "A":                  # keep the draw inside mode A's radius
                fl = fl.clamp(-5.9, 5.9)

            def run(cv):
                call("of_warp_bwd_det_cv", P(dout), P(f2), n, h, w, c, P(fl), P(dinp), P(dfl),
                     None, 0, cv, P(ws), wsb, st)
            us = {f: [] for f in FORMS}
            path = {}
            for cv, f in enumerate(FORMS):
                run(cv)
                torch.cuda.synchronize()
                path[f] = det_path(ws, hoff, n * h * w)
            for rnd in range(args.rounds):
                for cv, f in enumerate(FORMS):
                    e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                    e0.record()
                    for _ in range(args.reps):
                        run(cv)
                    e1.record()
                    torch.cuda.synchronize()
                    us[f].append(e0.elapsed_time(e1) / args.reps * 1e3)
            rec = {"level": lvl, "shape": [n, h, w, c], "flow_std": scale,
                   "path": {f: path[f][0] for f in FORMS}, "R": {f: path[f][1] for f in FORMS},
                   "us": {f: [round(v, 1) for v in us[f]] for f in FORMS},
                   "median_us": {f: round(float(np.median(us[f])), 1) for f in FORMS},
                   "reference_spread_us": round(spread(us["reference"]), 1)}
            out.append(rec)
            emit("det bwd level %d %3dx%3d c=%3d flow std %-4g | reference: path %-5s R %3d "
                 "%8.1f us | image: path %-5s R %3d %8.1f us | reference spread %.1f us" %
                 (lvl, h, w, c, scale, path["reference"][0], min(path["reference"][1], 999),
                  rec["median_us"]["reference"], path["image"][0], min(path["image"][1], 999),
                  rec["median_us"]["image"], rec["reference_spread_us"]))
    return out


def known_shifts(batch_size, height, width, seed):
    """(dx, dy) of every sample of data.synthetic_batch(batch_size, height, width, seed): the
    same generator calls in the same order."""
    rng = np.random.default_rng(seed)
    rng.random((batch_size, height, width, 3), dtype=np.float32)
    out = []
    for _ in range(batch_size):
        dy, dx = rng.integers(-4, 5, size=2)
        rng.normal(0.0, 0.01, (height, width, 3))
        out.append((int(dx), int(dy)))
    return out


def learn(args, emit):
    from optical_flow_amd.data import synthetic_batch
    h, w, b = args.learn_height, args.learn_width, args.learn_batch
    batch = torch.from_numpy(synthetic_batch(b, h, w, seed=args.learn_seed)).cuda()
    shifts = known_shifts(b, h, w, args.learn_seed)
    target = torch.tensor([[-dx / 2.0, -dy / 2.0] for dx, dy in shifts],
                          device="cuda").view(b, 1, 1, 2)
    emit("learn %dx%dx%d, %d steps, lr %g, shifts (dx, dy) %s; EPE of the H/2 flow against "
         "(-dx, -dy) / 2" % (b, h, w, args.learn_steps, args.learn_lr, shifts))
    res = {"shape": [b, h, w], "shifts": shifts, "curve": {}}
    for f in FORMS:
        tr = make_trainer(h, w, f, args.seed, args.learn_lr)
        curve = []
        for k in range(args.learn_steps + 1):
            loss, flows = tr.train_step(batch, k)
            if k % args.learn_every == 0 or k == args.learn_steps:
                epe = (flows[0] - target).norm(dim=-1).mean().item()
                curve.append([k, round(float(loss), 5), round(epe, 4)])
        res["curve"][f] = curve
        emit("learn %-9s (step, loss, EPE): %s" % (f, " ".join("(%d, %.4f, %.3f)" % tuple(c)
                                                              for c in curve)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40, help="steps per round and form")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=200, help="kernel launches per round and form")
    ap.add_argument("--mode-a-scales", type=float, nargs="*", default=[0.1, 1.0])
    ap.add_argument("--fixed-scale", type=float, default=6.0)
    ap.add_argument("--learn-height", type=int, default=192)
    ap.add_argument("--learn-width", type=int, default=256)
    ap.add_argument("--learn-batch", type=int, default=4)
    ap.add_argument("--learn-seed", type=int, default=1234)
    ap.add_argument("--learn-steps", type=int, default=200)
    ap.add_argument("--learn-every", type=int, default=20)
    ap.add_argument("--learn-lr", type=float, default=1e-4)
    ap.add_argument("--skip", nargs="*", default=[], choices=("step", "kernel", "learn"))
    ap.add_argument("--out", default=None, help="text report (the lines printed, then the JSON)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("warp_convention_ab.py measures on the GPU; none found")
    _lib.load()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit("# tools/warp_convention_ab.py: reference vs image warp convention, one process; "
         "device %s" % torch.cuda.get_device_name(0))
    res = {}
    if "step" not in args.skip:
        res["step"] = step_ab(args, emit)
    if "kernel" not in args.skip:
        res["kernel"] = kernel_ab(args, emit)
    if "learn" not in args.skip:
        res["learn"] = learn(args, emit)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
