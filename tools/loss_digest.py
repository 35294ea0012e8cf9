"""Digests of every loss entry's outputs, for a bitwise A/B of two trees (GPU).

python tools/loss_digest.py [--ssim] [--out loss_digest.txt]

Seeded inputs at the bench's loss size (384 x 512, B = 8, four levels of flows, scale 2).  For
every public loss entry of optical_flow_amd.ops and every combination of terms that takes a
path of its own (the rows of tests/test_gpu_loss_paths.py), in both warp conventions where the
entry has one, one line per output: the row, the convention, "loss" or "dflowK", and the
sha256 of the fp32 bytes.  Two trees compute the same loss iff their listings are equal line
for line (run both on the same machine: profiles/loss_unify_ab.md).
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, W, LEVELS = 8, 384, 512, 4


def _three(ops, b, f, **kw):
    return ops.census_flow_loss(b, f, 0.5, 3, 0.5, 0.2, 10, **kw)


def _ones(flows):
    return [torch.ones(f.shape[:3], device=f.device) for f in flows]


# (row, call(ops, batch, flows, convention keywords), takes a convention)
ROWS = [
    ("photometric_loss", lambda o, b, f, **c: o.photometric_loss(b, f, **c), True),
    ("flow_loss(0.2,10)", lambda o, b, f, **c: o.flow_loss(b, f, 0.2, 10, **c), True),
    ("flow_loss(0.0)", lambda o, b, f, **c: o.flow_loss(b, f, 0.0, **c), True),
    ("flow_smoothness(alpha=0)", lambda o, b, f: o.flow_smoothness(b, f, edge_alpha=0), False),
    ("flow_smoothness(alpha=10)", lambda o, b, f: o.flow_smoothness(b, f, edge_alpha=10), False),
    ("census_loss", lambda o, b, f, **c: o.census_loss(b, f, **c), True),
    ("census_flow_loss(three terms)", _three, True),
    ("census_flow_loss(photometric_weight=0)",
     lambda o, b, f, **c: o.census_flow_loss(b, f, 0.5, 3, 0.0, 0.2, 10, **c), True),
    ("census_flow_loss(three terms, weights=ones)",
     lambda o, b, f, **c: _three(o, b, f, weights=_ones(f), **c), True),
]
# the rows of the SSIM term (--ssim; a tree without the term has none of them)
SSIM_ROWS = [
    ("ssim_loss", lambda o, b, f, **c: o.ssim_loss(b, f, **c), True),
    ("census_flow_loss(0.15 L1 + 0.85 SSIM)",
     lambda o, b, f, **c: o.census_flow_loss(b, f, 0.0, photometric_weight=0.15,
                                             ssim_weight=0.85, **c), True),
    ("census_flow_loss(four terms)", lambda o, b, f, **c: _three(o, b, f, ssim_weight=0.7, **c),
     True),
    ("census_flow_loss(four terms, weights=ones)",
     lambda o, b, f, **c: _three(o, b, f, ssim_weight=0.7, weights=_ones(f), **c), True),
]


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ssim", action="store_true",
                    help="append the rows of the SSIM term (the other rows stay what they are)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loss_digest.py runs the loss kernels; no GPU is visible")
    from optical_flow_amd import _lib, ops
    from optical_flow_amd.data import synthetic_batch
    _lib.load()
    batch = torch.from_numpy(synthetic_batch(B, H, W, seed=1234)).cuda()
    rng = np.random.default_rng(77)
    flows = [torch.tensor(rng.standard_normal((B, H >> (s + 1), W >> (s + 1), 2)) * 2.0,
                          dtype=torch.float32).cuda() for s in range(LEVELS)]
    lines = []
    for row, fn, has_convention in ROWS + (SSIM_ROWS if args.ssim else []):
        for conv in (("reference", "image") if has_convention else ("-",)):
            fd = [f.clone().requires_grad_(True) for f in flows]
            loss = fn(ops, batch, fd, **({"convention": conv} if has_convention else {}))
            loss.backward()
            torch.cuda.synchronize()
            lines.append("%s | %s | loss | %s" % (row, conv, _sha(loss)))
            for k, f in enumerate(fd):
                lines.append("%s | %s | dflow%d | %s" % (row, conv, k, _sha(f.grad)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
