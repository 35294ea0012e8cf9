"""Evaluation against KITTI 2015 flow ground truth (build-added; the reference has no
evaluation): mean end-point error (EPE) and Fl-all of a net's flow.

A KITTI flow map (``training/flow_occ`` / ``flow_noc``) is a 16-bit RGB PNG: u = (R - 32768) / 64,
v = (G - 32768) / 64 in pixels of the native frame, valid where B != 0.  The net's finest flow
lives on an (H/2, W/2) grid in pixels of that grid; ``of_flow_eval`` (``flow_eval.hip``)
upsamples it to each map's native size, scales it to native pixels, compares and reduces in
one pass.  A pixel is an outlier when its error is above 3 px and above 5 % of the ground
truth's magnitude; Fl-all is the percentage of outliers among the valid pixels.

Only an image-convention net (``warp_convention="image"``) can be evaluated: a
reference-convention flow is not an image displacement (README, "warp convention").

    python -m optical_flow_amd.evaluate --kitti-flow ROOT --weights CKPT --height H --width W \\
        [--gt occ|noc] [--precision fp32|bf16] [--batch 8] [--write-flows DIR]
"""
from __future__ import annotations

import argparse
import collections
import concurrent.futures as cf
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np
import torch

from ._lib import call, lib

# the raw ground-truth batch (shared with the supervised loss term)
from .gt_raw import DESC_DTYPE, _upload, device_gt, pack_gt_raw  # noqa: F401


# ---- KITTI flow files -------------------------------------------------------------------------
def read_png_u16(path: str) -> np.ndarray:
    """A 16-bit RGB PNG as (h, w, 3) uint16, R, G, B, on the native decoder (of_png_read_u16);
    any other kind of PNG raises."""
    h, w = C.c_int(), C.c_int()
    call("of_png_info", os.fsencode(path), C.byref(h), C.byref(w), None, None)
    out = np.empty((h.value, w.value, 3), np.uint16)
    call("of_png_read_u16", os.fsencode(path), out.ctypes.data_as(C.c_void_p), out.size,
         C.byref(h), C.byref(w))
    return out


def write_png_u16(path: str, rgb: np.ndarray, filt: int = 5, level: int = 6):
    """(h, w, 3) uint16 R, G, B -> a 16-bit RGB PNG (of_png_write_u16)."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint16)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("expected (h, w, 3) samples, got shape %r" % (rgb.shape,))
    call("of_png_write_u16", os.fsencode(path), rgb.ctypes.data_as(C.c_void_p), rgb.shape[0],
         rgb.shape[1], filt | ((level + 1) << 8))


def decode_flow_kitti(rgb: np.ndarray):
    """The devkit's decode of a (h, w, 3) uint16 map: (flow float32 (h, w, 2), valid bool)."""
    flow = (rgb[:, :, :2].astype(np.float32) - np.float32(32768.0)) / np.float32(64.0)
    return flow, rgb[:, :, 2] != 0


def read_flow_kitti(path: str):
    """(flow float32 (h, w, 2), valid bool (h, w)) of a KITTI flow map."""
    return decode_flow_kitti(read_png_u16(path))


def encode_flow_kitti(flow, valid=None) -> np.ndarray:
    """q = clip(rint(f * 64 + 32768), 0, 65535) in R, G; B = 1 where valid (everywhere if None)."""
    flow = np.asarray(flow, dtype=np.float64)
    if flow.ndim != 3 or flow.shape[2] != 2:
        raise ValueError("expected a (h, w, 2) flow, got shape %r" % (flow.shape,))
    rgb = np.empty(flow.shape[:2] + (3,), np.uint16)
    rgb[:, :, :2] = np.clip(np.rint(flow * 64.0 + 32768.0), 0, 65535).astype(np.uint16)
    rgb[:, :, 2] = 1 if valid is None else (np.asarray(valid) != 0)
    return rgb


def write_flow_kitti(path: str, flow, valid=None):
    """Write a flow (h, w, 2) in KITTI's format; values outside the format's range clamp."""
    write_png_u16(path, encode_flow_kitti(flow, valid))


def list_kitti_flow(root: str, gt: str = "occ"):
    """Sorted [(image_2/N_10.png, image_2/N_11.png, flow_<gt>/N_10.png), ...] of a KITTI 2015
    flow tree; ``root`` is the dataset root holding ``training/`` or ``training/`` itself.
    Frames lacking any of the three files are skipped; no complete frame: FileNotFoundError."""
    if gt not in ("occ", "noc"):
        raise ValueError("gt must be 'occ' or 'noc', got %r" % (gt,))
    root = os.fspath(root)
    base = os.path.join(root, "training")
    if not os.path.isdir(base):
        base = root
    gdir, idir = os.path.join(base, "flow_" + gt), os.path.join(base, "image_2")
    frames = []
    if os.path.isdir(gdir) and os.path.isdir(idir):
        for name in sorted(os.listdir(gdir)):
            m = re.fullmatch(r"(\d+)_10\.png", name)
            if not m:
                continue
            trio = (os.path.join(idir, name), os.path.join(idir, m.group(1) + "_11.png"),
                    os.path.join(gdir, name))
            if all(os.path.isfile(p) for p in trio):
                frames.append(trio)
    if not frames:
        raise FileNotFoundError("no complete KITTI flow frame (image_2/N_10.png, image_2/N_11.png, "
                                "flow_%s/N_10.png) under %s" % (gt, base))
    return frames


def split_kitti_flow(frames, holdout_every: int):
    """(train, val) of list_kitti_flow's list: ``val`` is every ``holdout_every``-th frame of
    the sorted list (indices holdout_every - 1, 2 * holdout_every - 1, ...), ``train`` the
    rest, both in sorted order."""
    if isinstance(holdout_every, bool) or int(holdout_every) != holdout_every or holdout_every < 2:
        raise ValueError("holdout_every must be an integer >= 2, got %r" % (holdout_every,))
    frames = sorted(tuple(f) for f in frames)
    k = int(holdout_every)
    val = [f for i, f in enumerate(frames) if (i + 1) % k == 0]
    train = [f for i, f in enumerate(frames) if (i + 1) % k != 0]
    return train, val


class KittiFlowReader:
    """Labelled batches of a KITTI 2015 flow tree for supervised fine-tuning: iterating yields
    ``(batch, gt_raw, descs)`` -- the (B, H, W, 6) CUDA batch of_preprocess_pairs makes of the
    frames, and pack_gt_raw's ground-truth buffer (on the GPU) with its host descriptors, which
    Trainer.train_step takes as ``gt=(gt_raw, descs)``.

    Every iteration is one epoch: the frames in a seeded shuffle of their own (``order``), the
    last short batch dropped.  Frames and maps are decoded ``nworkers`` at a time, up to two
    batches ahead, as evaluate() does; both go up by asynchronous copies from pinned staging.
    The reader's own ``augment`` (AsyncReader's keyword) would move the frames and leave the
    ground truth behind, so anything but None raises ValueError.  ``label_augment`` (an
    AugmentOpts) moves both: batch k of epoch e draws ``records(e, k)``, the frames go through
    of_augment_pairs in place of of_preprocess_pairs and the maps through of_gt_augment with the
    same records (ops.augment_gt; DESIGN.md "Labelled augmentation").  With None, the default,
    nothing changes and neither kernel is launched."""

    def __init__(self, frames_or_root, batch_size: int, img_height: int, img_width: int,
                 gt: str = "occ", nworkers: int = 6, seed: int = 0, augment=None,
                 label_augment=None):
        if augment is not None:
            raise ValueError("labelled KITTI flow frames are not augmented (AugmentOpts given): a "
                             "crop, zoom or flip would have to move the ground truth with it")
        if label_augment is not None:
            from .data_reader import AugmentOpts
            if not isinstance(label_augment, AugmentOpts):
                raise TypeError("label_augment must be an AugmentOpts or None, got %r"
                                % (type(label_augment),))
        self.label_augment = label_augment
        if isinstance(frames_or_root, (str, os.PathLike)):
            frames = list_kitti_flow(frames_or_root, gt)
        else:
            frames = [tuple(f) for f in frames_or_root]
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1, got %r" % (batch_size,))
        if len(frames) < batch_size:
            raise ValueError("%d labelled frames do not fill one batch of %d"
                             % (len(frames), batch_size))
        self.frames = frames
        self.batch_size = int(batch_size)
        self.height, self.width = int(img_height), int(img_width)
        self.nworkers = max(1, int(nworkers))
        self.seed = int(seed)
        self.nbatches = len(frames) // self.batch_size
        self.epoch = 0

    def order(self, epoch: int):
        """The frame indices of ``epoch`` in reading order: a permutation seeded by (seed,
        epoch), cut to whole batches."""
        perm = np.random.default_rng([self.seed, int(epoch)]).permutation(len(self.frames))
        return [int(i) for i in perm[:self.nbatches * self.batch_size]]

    def records(self, epoch: int, k: int):
        """The of_augment records of batch ``k`` of ``epoch`` (label_augment only):
        sample_augment seeded by (seed, epoch * nbatches + k), one record per frame, shared by
        the frame's two images and its ground-truth map."""
        if self.label_augment is None:
            raise ValueError("records() needs a reader built with label_augment")
        if not 0 <= int(k) < self.nbatches or int(epoch) < 0:
            raise ValueError("batch %r of epoch %r: the reader has %d batches per epoch"
                             % (k, epoch, self.nbatches))
        from .data_reader import sample_augment
        return sample_augment(self.label_augment, self.batch_size, self.height, self.width,
                              self.seed, int(epoch) * self.nbatches + int(k))

    def host_batches(self, epoch: int):
        """The epoch's batches on the host: (pairs, maps, indices) per batch -- BGR uint8 frame
        pairs, (h, w, 3) uint16 maps, the frames' indices.  No GPU work."""
        order = self.order(epoch)
        pending = collections.deque()
        todo = iter(order)
        with cf.ThreadPoolExecutor(self.nworkers) as pool:
            def fill():
                while len(pending) < 2 * self.batch_size:
                    i = next(todo, None)
                    if i is None:
                        return
                    pending.append((i, pool.submit(_decode_frame, self.frames[i])))
            fill()
            while pending:
                pairs, maps, idx = [], [], []
                while len(pairs) < self.batch_size:
                    i, fut = pending.popleft()
                    (img1, img2, gmap), _ = fut.result()
                    pairs.append((img1, img2))
                    maps.append(gmap)
                    idx.append(i)
                    fill()
                yield pairs, maps, idx

    def __iter__(self):
        from .data_reader import _pack_raw
        epoch, self.epoch = self.epoch, self.epoch + 1
        for k, (pairs, maps, _) in enumerate(self.host_batches(epoch)):
            dev = _upload(_pack_raw(pairs))
            batch = torch.empty((len(pairs), self.height, self.width, 6), device="cuda")
            if self.label_augment is not None:
                yield self._augmented(epoch, k, dev, batch, maps)
                continue
            call("of_preprocess_pairs", C.c_void_p(dev.data_ptr()), len(pairs), self.height,
                 self.width, C.c_void_p(batch.data_ptr()), _stream())
            raw, descs = pack_gt_raw(maps)
            yield batch, _upload(raw), descs

    def _augmented(self, epoch, k, dev, batch, maps):
        """One batch of the label_augment path: the raw frames ``dev`` into ``batch`` through
        records(epoch, k), and the maps through the same records."""
        from . import ops
        rec = _upload(self.records(epoch, k).view(np.uint8))
        call("of_augment_pairs", C.c_void_p(dev.data_ptr()), batch.shape[0], self.height,
             self.width, C.c_void_p(rec.data_ptr()), C.c_void_p(batch.data_ptr()), _stream())
        raw, descs = pack_gt_raw(maps)
        gt_raw, descs = ops.augment_gt((_upload(raw), descs), rec, (self.height, self.width))
        return batch, gt_raw, descs


# ---- device ops -------------------------------------------------------------------------------
def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _flow_arg(flow):
    if not (torch.is_tensor(flow) and flow.is_cuda and flow.dim() == 4 and flow.shape[3] == 2):
        raise ValueError("expected a CUDA flow tensor (n, fh, fw, 2), got %r" %
                         (tuple(flow.shape) if torch.is_tensor(flow) else type(flow),))
    return flow.detach().float().contiguous()


def flow_metrics(flow: torch.Tensor, gt_raw, descs=None):
    """of_flow_eval: per-image (sum_epe float64, n_valid int64, n_outlier int64) CUDA tensors of
    ``flow`` (n, fh, fw, 2) against ``gt_raw`` -- a list of n (h, w, 3) uint16 maps, or
    pack_gt_raw's buffer (numpy or already on the GPU) with its descriptors.  Stream-ordered:
    host ground truth is uploaded by an asynchronous copy from pinned staging, and nothing is
    read back."""
    flow = _flow_arg(flow)
    n, fh, fw = flow.shape[:3]
    gt_raw, descs = device_gt(gt_raw, descs, n)
    npart = lib().of_flow_eval_partials(n, int(descs["h"].max(initial=1)),
                                        int(descs["w"].max(initial=1)))
    partials = torch.empty(max(3 * npart, 1), dtype=torch.float64, device="cuda")
    out = torch.empty((max(n, 1), 3), dtype=torch.int64, device="cuda")
    call("of_flow_eval", C.c_void_p(flow.data_ptr()), n, fh, fw, C.c_void_p(gt_raw.data_ptr()),
         descs.ctypes.data_as(C.c_void_p), gt_raw.numel(), C.c_void_p(partials.data_ptr()), npart,
         C.c_void_p(out.data_ptr()), _stream())
    out = out[:n]
    return out[:, 0].view(torch.float64), out[:, 1], out[:, 2]


def upsample_flow(flow: torch.Tensor, gh: int, gw: int) -> torch.Tensor:
    """of_flow_upsample: (n, fh, fw, 2) on its own grid -> (n, gh, gw, 2) in pixels of the
    gh x gw image (the sampling of_flow_eval compares)."""
    flow = _flow_arg(flow)
    n, fh, fw = flow.shape[:3]
    out = torch.empty((n, int(gh), int(gw), 2), dtype=torch.float32, device="cuda")
    call("of_flow_upsample", C.c_void_p(flow.data_ptr()), n, fh, fw, int(gh), int(gw),
         C.c_void_p(out.data_ptr()), _stream())
    return out


def _check_convention(net):
    cv = getattr(net, "warp_convention", "reference")
    if cv != "image":
        raise ValueError("evaluation needs a net built with warp_convention='image' (this one is "
                         "%r): a reference-convention flow is not an image displacement" % (cv,))


def _finest_flow(net, frames):
    """The net's finest flow for [(img1_bgr_u8, img2_bgr_u8), ...] at any native size."""
    from .data_reader import _pack_raw
    with torch.no_grad():
        # preprocess_frames with the upload of _upload (no host wait on the copy)
        dev = _upload(_pack_raw(frames))
        batch = torch.empty((len(frames), net.height, net.width, 6), device="cuda")
        call("of_preprocess_pairs", C.c_void_p(dev.data_ptr()), len(frames), net.height,
             net.width, C.c_void_p(batch.data_ptr()), _stream())
        return net(batch)[0].detach()


def predict_flow(net, img1_bgr: np.ndarray, img2_bgr: np.ndarray) -> torch.Tensor:
    """The flow from image 1 to image 2 at the frames' native size: (h, w, 2) float32 CUDA, x
    and y displacement in native pixels.  The frames (uint8 BGR, any size) are resized to the
    net's H x W as in training; no gradient is recorded."""
    _check_convention(net)
    if img1_bgr.shape != img2_bgr.shape:
        raise ValueError("the two frames differ in shape: %r and %r" %
                         (img1_bgr.shape, img2_bgr.shape))
    flow = _finest_flow(net, [(img1_bgr, img2_bgr)])
    return upsample_flow(flow, img1_bgr.shape[0], img1_bgr.shape[1])[0]


def _decode_frame(trio):
    from .data_reader import imread_bgr
    t0 = time.perf_counter()
    out = imread_bgr(trio[0]), imread_bgr(trio[1]), read_png_u16(trio[2])
    return out, time.perf_counter() - t0


def evaluate(net, frames_or_root, gt: str = "occ", batch_size: int = 8, nworkers: int = 6,
             write_flows: str = None):
    """EPE and Fl-all of ``net`` over a KITTI flow tree (or list_kitti_flow's list).

    The frames and maps are decoded ``nworkers`` at a time (the native calls release the GIL),
    up to two batches ahead of the GPU; each batch is one forward under no_grad and one
    of_flow_eval; frames and maps go up by asynchronous copies from pinned staging and the
    per-image sums stay on the GPU, so the host waits for the GPU once, at the read-back at the
    end (beyond what the host allocator does when its pinned pool has to grow).  The last
    partial batch is evaluated.  Training state is left alone (no gradient, no weight, no
    ``store.version`` change).  Returns a dict:
      epe, fl_all           mean over the images of the per-image mean EPE (px) / of
                            100 * n_outlier / n_valid (the devkit's averaging); None when every
                            image is empty
      epe_pooled, fl_pooled the same over all valid pixels
      n_images, n_valid     images evaluated, valid pixels
      n_images_empty        images with no valid pixel: in n_images, not in the image means
      per_image             {"sum_epe", "n_valid", "n_outlier"}: arrays over the images
      timing                {"total_s", "decode_s" (summed over the decode threads), "wait_s"
                            (the main thread blocked on decodes)}
    write_flows: a directory that receives each prediction as a KITTI-format PNG named like its
    ground-truth file (this mode reads every batch back)."""
    _check_convention(net)
    if isinstance(frames_or_root, (str, os.PathLike)):
        frames = list_kitti_flow(frames_or_root, gt)
    else:
        frames = [tuple(f) for f in frames_or_root]
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1, got %r" % (batch_size,))
    if not frames:
        raise ValueError("no frames to evaluate")
    if write_flows:
        os.makedirs(write_flows, exist_ok=True)
    t_start = time.perf_counter()
    decode_s = wait_s = 0.0
    results = []
    pending = collections.deque()
    todo = iter(frames)
    with cf.ThreadPoolExecutor(max(1, int(nworkers))) as pool:
        def fill():
            while len(pending) < 2 * batch_size:
                trio = next(todo, None)
                if trio is None:
                    return
                pending.append((trio, pool.submit(_decode_frame, trio)))
        fill()
        while pending:
            pairs, maps, names = [], [], []
            while pending and len(pairs) < batch_size:
                trio, fut = pending.popleft()
                t0 = time.perf_counter()
                (img1, img2, gmap), dt = fut.result()
                wait_s += time.perf_counter() - t0
                decode_s += dt
                pairs.append((img1, img2))
                maps.append(gmap)
                names.append(os.path.basename(trio[2]))
                fill()
            flow = _finest_flow(net, pairs)
            s, v, o = flow_metrics(flow, maps)
            results.append(torch.stack((s, v.double(), o.double()), 1))   # counts exact in double
            if write_flows:
                for k, (m, name) in enumerate(zip(maps, names)):
                    up = upsample_flow(flow[k:k + 1], m.shape[0], m.shape[1])[0]
                    write_flow_kitti(os.path.join(write_flows, name), up.cpu().numpy())
    res = torch.cat(results).cpu().numpy()                # the one read-back (float64)
    sum_epe = res[:, 0].copy()
    n_valid = np.rint(res[:, 1]).astype(np.int64)
    n_outlier = np.rint(res[:, 2]).astype(np.int64)
    out = summarise(sum_epe, n_valid, n_outlier)
    out["timing"] = {"total_s": time.perf_counter() - t_start, "decode_s": decode_s,
                     "wait_s": wait_s}
    return out


def summarise(sum_epe, n_valid, n_outlier):
    """The result dict of evaluate() from the per-image sums (numpy, any float / int type)."""
    sum_epe = np.asarray(sum_epe, np.float64)
    n_valid = np.asarray(n_valid, np.int64)
    n_outlier = np.asarray(n_outlier, np.int64)
    some = n_valid > 0
    nv = n_valid[some].astype(np.float64)
    total = int(n_valid.sum())
    return {
        "epe": float(np.mean(sum_epe[some] / nv)) if some.any() else None,
        "fl_all": float(np.mean(100.0 * n_outlier[some] / nv)) if some.any() else None,
        "epe_pooled": float(sum_epe.sum() / total) if total else None,
        "fl_pooled": float(100.0 * n_outlier.sum() / total) if total else None,
        "n_images": int(len(n_valid)),
        "n_images_empty": int((~some).sum()),
        "n_valid": total,
        "per_image": {"sum_epe": sum_epe, "n_valid": n_valid, "n_outlier": n_outlier},
    }


def to_json(result) -> str:
    """One JSON line of evaluate()'s dict (arrays as lists)."""
    rec = dict(result)
    rec["per_image"] = {k: np.asarray(v).tolist() for k, v in result["per_image"].items()}
    return json.dumps(rec)


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--kitti-flow", required=True, metavar="ROOT",
                    help="KITTI 2015 flow root (holding training/) or training/ itself")
    ap.add_argument("--weights", default=None,
                    help="the whole net's weights as save_weights / train --save-dir wrote them: a "
                         "TensorFlow checkpoint prefix or an .npz; every tensor must be present "
                         "(default: the seeded initial net)")
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--gt", default="occ", choices=("occ", "noc"))
    ap.add_argument("--precision", default="fp32", choices=("fp32", "bf16"))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--nworkers", type=int, default=6)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--write-flows", default=None, metavar="DIR",
                    help="write every prediction as a KITTI-format PNG into DIR")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    from .model import build_flow_net
    frames = list_kitti_flow(args.kitti_flow, args.gt)
    net = build_flow_net(args.height, args.width, seed=args.seed, precision=args.precision,
                         warp_convention="image")
    if args.weights is not None:
        # the whole net, every tensor (strict): what train --save-dir / save_weights wrote.
        # (build_flow_net's own path argument is the stand-alone encoder's loader.)
        net.load_weights(args.weights, strict=True)
    res = evaluate(net, frames, batch_size=args.batch, nworkers=args.nworkers,
                   write_flows=args.write_flows)
    res["gt"] = args.gt
    print(to_json(res), flush=True)


if __name__ == "__main__":
    main()
