"""Cost of the KITTI flow evaluation (GPU; DESIGN.md §3 "Evaluation").

python tools/eval_cost.py [--rounds 20] [--iters 50] [--frames 200] [--out eval_cost.json]

Part 1, the metric alone, at (96, 320) -> 375 x 1242 with n = 8 (a 192 x 640 net's finest flow
against KITTI-size maps), two arms in one process on one card, alternated round by round, each
round ``--iters`` calls between one device event pair, after warm-up rounds:
  fused   of_flow_eval (flow_eval.hip): upsampling, decode, error and reduction in one pass;
  torch   the same metric composed from torch ops: F.interpolate(bilinear, align_corners=False),
          the scaling, the uint16 decode, the error, the 3 px / 5 % rule and the sums.
Both arms cycle over ``--buffers`` distinct ground-truth batches (16 x 22.4 MB by default, more
than the 256 MB last-level cache), so a call reads its maps from HBM as an evaluation does.
Bytes per fused call = the maps (6 bytes per pixel) + the flow once: the bytes the algorithm
needs, computed from the shapes, not a counter reading (profiles/r6_summary.md reports counter
values, "HBM MB / launch (PMC)", and states no peak).  The achieved rate is that byte count over
the median call time, given against the MI355X's 8.0 TB/s HBM3E specification peak; both the
byte count and the peak figure are this tool's own choice.

Part 2, evaluate() end to end on a synthetic tree of ``--frames`` frames of KITTI's four sizes
(random images, random valid ground truth, written with the project's encoder into a temporary
directory): wall time, the decode threads' summed time, and the time the main thread waited
for decodes.  ``--frames 0`` skips it.

Prints one JSON line.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # bytes / s, MI355X HBM3E
KITTI_SIZES = [(375, 1242), (370, 1224), (374, 1238), (376, 1241)]


def random_map(h, w, rng):
    """A KITTI-format map: about 30 % valid, ground truth within +-60 px."""
    rgb = np.zeros((h, w, 3), np.uint16)
    rgb[:, :, :2] = rng.integers(32768 - 3840, 32768 + 3840, (h, w, 2))
    rgb[:, :, 2] = rng.uniform(size=(h, w)) < 0.3
    return rgb


def torch_metric(flow, gt16, gh, gw):
    """flow (n, fh, fw, 2) fp32; gt16 (n, gh, gw, 3) int16 (the uint16 samples' bits)."""
    n, fh, fw = flow.shape[:3]
    up = F.interpolate(flow.permute(0, 3, 1, 2), size=(gh, gw), mode="bilinear",
                       align_corners=False)
    u, v = up[:, 0] * (gw / fw), up[:, 1] * (gh / fh)
    g = gt16.to(torch.float32)
    g = torch.where(g < 0, g + 65536.0, g)
    gu, gv = (g[..., 0] - 32768.0) / 64.0, (g[..., 1] - 32768.0) / 64.0
    valid = gt16[..., 2] != 0
    epe = torch.sqrt((u - gu) ** 2 + (v - gv) ** 2)
    outlier = valid & (epe > 3.0) & (epe > 0.05 * torch.sqrt(gu * gu + gv * gv))
    return ((epe * valid).double().sum((1, 2)), valid.sum((1, 2)), outlier.sum((1, 2)))


def time_metric(args):
    from optical_flow_amd.evaluate import flow_metrics, pack_gt_raw
    fh, fw, gh, gw, n = 96, 320, 375, 1242, 8
    rng = np.random.default_rng(0)
    flow = torch.from_numpy(rng.uniform(-8, 8, (n, fh, fw, 2)).astype(np.float32)).cuda()
    raws, stacks = [], []
    for _ in range(args.buffers):
        maps = [random_map(gh, gw, rng) for _ in range(n)]
        raw, desc = pack_gt_raw(maps)
        raws.append((torch.from_numpy(raw).cuda(), desc))
        stacks.append(torch.from_numpy(np.stack(maps).view(np.int16)).cuda())
    arms = {
        "fused": lambda k: flow_metrics(flow, raws[k][0], raws[k][1]),
        "torch": lambda k: torch_metric(flow, stacks[k], gh, gw),
    }
    # the two arms compute the same metric: equal counts up to pixels within rounding of a
    # threshold (random inputs keep no margin), sums within rounding
    a, b = arms["fused"](0), arms["torch"](0)
    agree = {"sum_epe_rel": float(((a[0] - b[0]).abs() / b[0]).max()),
             "n_valid_equal": bool(torch.equal(a[1], b[1])),
             "n_outlier_maxdiff": int((a[2] - b[2]).abs().max())}
    times = {k: [] for k in arms}
    for r in range(args.warmup + args.rounds):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(args.iters):
                fn((r * args.iters + i) % args.buffers)
            e1.record()
            e1.synchronize()
            if r >= args.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3 / args.iters)     # us per call
    rec = {"shape": {"flow": [n, fh, fw, 2], "gt": [n, gh, gw, 3]}, "agreement": agree, "arms": {}}
    for name, t in times.items():
        q = np.percentile(t, [25, 50, 75])
        rec["arms"][name] = {"median_us": round(float(q[1]), 2), "q25_us": round(float(q[0]), 2),
                             "q75_us": round(float(q[2]), 2), "min_us": round(float(min(t)), 2)}
    nbytes = n * gh * gw * 6 + flow.numel() * 4
    rec["fused_bytes"] = nbytes
    rate = nbytes / (rec["arms"]["fused"]["median_us"] * 1e-6)
    rec["fused_bytes_per_s"] = round(rate, -6)
    rec["fused_hbm_peak_fraction"] = round(rate / HBM_PEAK, 4)
    rec["torch_over_fused"] = round(rec["arms"]["torch"]["median_us"] /
                                    rec["arms"]["fused"]["median_us"], 2)
    return rec


def time_evaluate(args):
    from optical_flow_amd.data_reader import imwrite
    from optical_flow_amd.evaluate import evaluate, write_png_u16
    from optical_flow_amd.model import FlowNet
    rng = np.random.default_rng(1)
    root = tempfile.mkdtemp(prefix="kitti_flow_synth_")
    try:
        for d in ("image_2", "flow_occ"):
            os.makedirs(os.path.join(root, "training", d))
        for k in range(args.frames):
            h, w = KITTI_SIZES[k % len(KITTI_SIZES)]
            for tag in ("10", "11"):
                imwrite(os.path.join(root, "training", "image_2", "%06d_%s.png" % (k, tag)),
                        rng.integers(0, 256, (h, w, 3)).astype(np.uint8))
            write_png_u16(os.path.join(root, "training", "flow_occ", "%06d_10.png" % k),
                          random_map(h, w, rng))
        net = FlowNet(192, 640, warp_convention="image")
        runs = []
        for _ in range(3):                       # the first run warms the kernels and the files
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = evaluate(net, root, batch_size=args.batch, nworkers=args.nworkers)
            torch.cuda.synchronize()
            runs.append({"wall_s": round(time.perf_counter() - t0, 3),
                         "decode_thread_s": round(res["timing"]["decode_s"], 3),
                         "wait_for_decode_s": round(res["timing"]["wait_s"], 3)})
        return {"frames": args.frames, "batch": args.batch, "nworkers": args.nworkers,
                "net": [192, 640], "runs": runs, "epe": res["epe"], "fl_all": res["fl_all"]}
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20, help="timed rounds per arm")
    ap.add_argument("--warmup", type=int, default=3, help="untimed rounds per arm")
    ap.add_argument("--iters", type=int, default=50, help="calls per round")
    ap.add_argument("--buffers", type=int, default=16, help="distinct ground-truth batches")
    ap.add_argument("--frames", type=int, default=200, help="frames of the synthetic tree")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--nworkers", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_cost.py measures on the GPU; none is visible")
    from optical_flow_amd import _lib
    _lib.load()
    rec = {"metric": time_metric(args)}
    if args.frames > 0:
        rec["evaluate"] = time_evaluate(args)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
