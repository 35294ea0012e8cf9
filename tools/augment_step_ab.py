#!/usr/bin/env python
"""Step time of the training driver on a KITTI-shaped tree with and without --augment, in one
call: the two forms alternate (plain, augment, plain, augment, ...), each run a fresh
`python -m optical_flow_amd.train --kitti TREE --log ...` process, and the step time is read
from the JSONL log (the driver reads the loss back every step, so consecutive "t" stamps are a
step apart).  The first epoch of each run (start-up, first launches) is left out.

The tree: one drive of --frames synthetic 375x1242 frames per camera (tools/data_bench.py's
frames), i.e. 2 * frames - 1 pairs.  Prints one JSON line (and writes it to --out when given).
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def make_tree(root, frames):
    from data_bench import synth_frame
    from optical_flow_amd.data_reader import imwrite
    rng = np.random.default_rng(0)
    open_dirs = []
    for cam in ("image_02", "image_03"):
        d = os.path.join(root, "2011_09_26", "2011_09_26_drive_0001_sync", cam, "data")
        os.makedirs(d)
        open_dirs.append(d)
    for f in range(frames):
        for d in open_dirs:
            imwrite(os.path.join(d, "%010d.png" % f), synth_frame(rng, 375, 1242))


def step_times(log_path):
    """Per-step seconds of every epoch but the first ("t" restarts at each epoch)."""
    recs = [json.loads(l) for l in open(log_path) if l.strip()]
    t = [r["t"] for r in recs if "step" in r]
    starts = [i for i in range(len(t)) if i == 0 or t[i] < t[i - 1]]
    out = []
    for a, b in zip(starts[1:], starts[2:] + [len(t)]):
        out += list(np.diff(t[a:b]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--nworkers", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="ofaug_")
    tree = os.path.join(tmp, "kitti")
    make_tree(tree, args.frames)
    res = {"tree": "%d pairs of 375x1242 frames" % (2 * args.frames - 1), "batch": args.batch,
           "out": [args.height, args.width], "epochs": args.epochs, "runs": []}
    for rnd in range(args.rounds):
        for form, extra in (("plain", []), ("augment", ["--augment"])):
            log = os.path.join(tmp, "%s_%d.jsonl" % (form, rnd))
            cmd = [sys.executable, "-m", "optical_flow_amd.train", "--kitti", tree, "--height",
                   str(args.height), "--width", str(args.width), "--batch", str(args.batch),
                   "--epochs", str(args.epochs), "--nworkers", str(args.nworkers), "--log",
                   log] + extra
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit("%s failed (%d):\n%s" % (" ".join(cmd), r.returncode, r.stderr[-2000:]))
            dt = step_times(log)
            res["runs"].append({"form": form, "round": rnd, "steps": len(dt),
                                "median_ms": round(float(np.median(dt)) * 1e3, 3),
                                "mean_ms": round(float(np.mean(dt)) * 1e3, 3)})
    for form in ("plain", "augment"):
        res[form + "_median_ms"] = [r["median_ms"] for r in res["runs"] if r["form"] == form]
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
