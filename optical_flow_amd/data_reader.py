"""KITTI data path (SURVEY.md §8 f row 1): the reference ``data_reader.py`` with the same names
and argument meaning, on the native reader (``reader.cpp``: PNG decode threads, pinned batch
slots) and the HIP preprocess kernel (``image_ops.hip``: cv2-style resize + normalise + pair
packing in HBM).

Differences from the reference, by design:
  - ``get_batch()`` returns the ``(B, H, W, 6)`` float32 batch already on the GPU (the
    reference returns numpy and ``train.py:75`` converts it); the host->device copy moves the
    8-bit frames at their native size, on a side HIP stream.
  - Batches come out in submission order and the shuffle / pair swaps are seeded
    (``ReaderOpts.seed``), so a run is reproducible; the reference's Pool queue delivers in
    completion order with unseeded ``random`` / ``np.random``.
  - Worker threads in one process instead of a ``multiprocessing.Pool`` (no cv2 fork issue to
    work around: ``data_reader.py:104-106``).
  - Seeded training augmentation (``AugmentOpts`` / ``ReaderOpts(augment=...)``; the reference
    stops at ``# TODO: Data augmentation``, ``train.py:13``): random zoom / crop, horizontal
    flip, rotation and colour jitter, in the HIP kernel that otherwise does the resize
    (``augment.hip``).  Off by default.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import call

image_means = (np.array([123.0, 117.0, 104.0]) / 255.0).reshape(1, 1, 3)   # data_reader.py:7-9


def _drive_dirs(kitti_path: str):
    """(left camera dir, right camera dir) of every drive, days and drives in os.listdir
    order; a day's calibration files (names ending in '.txt') are not drives."""
    for day in os.listdir(kitti_path):
        day_dir = os.path.join(kitti_path, day)
        for drive in os.listdir(day_dir):
            if not drive.endswith(".txt"):
                cams = [os.path.join(day_dir, drive, cam, "data") for cam in ("image_02", "image_03")]
                assert all(os.path.isdir(c) for c in cams), "missing camera dir in %s" % drive
                yield cams


def _drive_pairs(left: str, right: str) -> List[List[str]]:
    """One drive's pairs: consecutive left frames (temporal), then each left frame with the
    right frame of the same name (stereo); frames in sorted-name order."""
    names = sorted(os.listdir(left))
    lpaths = [os.path.join(left, f) for f in names]
    temporal = [[a, b] for a, b in zip(lpaths, lpaths[1:])]
    rpaths = [os.path.join(right, f) for f in names]
    assert all(os.path.isfile(r) for r in rpaths), "right frame missing under %s" % right
    return temporal + [[a, b] for a, b in zip(lpaths, rpaths)]


def read_kitti(kitti_path: str) -> List[List[str]]:
    """The pair list of data_reader.py:12-32 -- per drive, the temporal pairs (image_02
    frames i, i+1) then the stereo pairs (image_02 / image_03 frame i) -- with the same
    listing order, asserts and the printed total."""
    pairs = [p for left, right in _drive_dirs(kitti_path) for p in _drive_pairs(left, right)]
    print("Total number of KITTI pairs: %d" % len(pairs))
    return pairs


# of_augment (include/oflow.h): one 64-byte record per pair
AUGMENT_DTYPE = np.dtype([("m", np.float32, (6,)), ("gain", np.float32, (3,)),
                          ("brightness", np.float32), ("contrast", np.float32),
                          ("saturation", np.float32), ("flags", np.int32),
                          ("pad", np.int32, (3,))])
assert AUGMENT_DTYPE.itemsize == 64


def _range(name, v, lo_min=None):
    try:
        lo, hi = (float(x) for x in v)
    except (TypeError, ValueError):
        raise ValueError("%s must be a (lo, hi) pair, got %r" % (name, v))
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError("%s must be finite, got %r" % (name, v))
    if lo > hi:
        raise ValueError("%s needs lo <= hi, got %r" % (name, v))
    if lo_min is not None and lo < lo_min:
        raise ValueError("%s must start at >= %g, got %r" % (name, lo_min, v))
    return lo, hi


def _amplitude(name, v):
    v = float(v)
    if not (math.isfinite(v) and v >= 0):
        raise ValueError("%s must be finite and >= 0, got %r" % (name, v))
    return v


class AugmentOpts:
    """Training augmentation of the KITTI batch (sample_augment draws from these; both images of
    a pair get the same draw):
      zoom         range of z >= 1; the crop window is 1/z of the frame on each axis
      translate    window position uniform over the slack the zoom leaves (else centred)
      hflip_prob   probability of a horizontal flip
      rotate_deg   angle uniform in +-that, about the output centre, in output-pixel space
                   (samples that leave the frame replicate its border)
      brightness   delta uniform in +-that, added to the [0, 1] pixel value
      contrast     range of the factor about 0.5
      saturation   range of the factor about the pixel's gray
      color_gain   range of the per-channel multiplier, drawn per channel
    Every default is the identity; ValueError for a range with lo > hi, zoom below 1, a
    probability outside [0, 1] or a non-finite value."""

    def __init__(self, zoom=(1.0, 1.0), translate=True, hflip_prob=0.0, rotate_deg=0.0,
                 brightness=0.0, contrast=(1.0, 1.0), saturation=(1.0, 1.0),
                 color_gain=(1.0, 1.0)):
        self.zoom = _range("zoom", zoom, lo_min=1.0)
        self.translate = bool(translate)
        hflip_prob = float(hflip_prob)
        if not 0.0 <= hflip_prob <= 1.0:                  # refuses NaN too
            raise ValueError("hflip_prob must be in [0, 1], got %r" % (hflip_prob,))
        self.hflip_prob = hflip_prob
        self.rotate_deg = _amplitude("rotate_deg", rotate_deg)
        self.brightness = _amplitude("brightness", brightness)
        self.contrast = _range("contrast", contrast)
        self.saturation = _range("saturation", saturation)
        self.color_gain = _range("color_gain", color_gain)

    @property
    def has_color(self) -> bool:
        """Some colour range is non-trivial (the records then carry flags bit 0)."""
        return (self.brightness != 0.0 or self.contrast != (1.0, 1.0) or
                self.saturation != (1.0, 1.0) or self.color_gain != (1.0, 1.0))

    def as_dict(self):
        return {"zoom": list(self.zoom), "translate": self.translate,
                "hflip_prob": self.hflip_prob, "rotate_deg": self.rotate_deg,
                "brightness": self.brightness, "contrast": list(self.contrast),
                "saturation": list(self.saturation), "color_gain": list(self.color_gain)}


def sample_augment(opts: AugmentOpts, batch_size: int, out_h: int, out_w: int, seed: int,
                   batch_index: int) -> np.ndarray:
    """The of_augment records of one batch: a (batch_size,) array of AUGMENT_DTYPE.

    Draws from ``np.random.default_rng([seed, batch_index])``, so batch k's records depend on
    (seed, k) alone.  Every draw below is made for every batch, used or not, in this order,
    each a vector over the batch: zoom z; window position tx, ty in [0, 1); flip (a uniform
    number < hflip_prob); angle; brightness; contrast; saturation; colour gain (batch x 3).

    The map from the output pixel centre (xc, yc) to the normalised source position is built in
    float64 and cast to float32 at the end: centre (xc - W/2, yc - H/2), flip (x -> -x), rotate
    by the angle, scale by 1/z, translate by the window centre (W/(2z) + tx W (1 - 1/z), the
    same in y; tx = ty = 0.5 without ``translate``), divide by (W, H)."""
    B, W, H = int(batch_size), float(out_w), float(out_h)
    rng = np.random.default_rng([int(seed), int(batch_index)])
    z = rng.uniform(opts.zoom[0], opts.zoom[1], B)
    tx, ty = rng.uniform(0.0, 1.0, B), rng.uniform(0.0, 1.0, B)
    flip = rng.uniform(0.0, 1.0, B) < opts.hflip_prob
    ang = np.deg2rad(rng.uniform(-opts.rotate_deg, opts.rotate_deg, B))
    bright = rng.uniform(-opts.brightness, opts.brightness, B)
    contrast = rng.uniform(opts.contrast[0], opts.contrast[1], B)
    sat = rng.uniform(opts.saturation[0], opts.saturation[1], B)
    gain = rng.uniform(opts.color_gain[0], opts.color_gain[1], (B, 3))
    if not opts.translate:
        tx = ty = np.full(B, 0.5)
    sgn = np.where(flip, -1.0, 1.0)
    c, s = np.cos(ang), np.sin(ang)
    # rows of (rotation x flip) / z, then the centre shift and the window centre
    a00, a01 = c * sgn / z, -s / z
    a10, a11 = s * sgn / z, c / z
    cx = W / (2.0 * z) + tx * (W * (1.0 - 1.0 / z))
    cy = H / (2.0 * z) + ty * (H * (1.0 - 1.0 / z))
    a02 = a00 * (-W / 2.0) + a01 * (-H / 2.0) + cx
    a12 = a10 * (-W / 2.0) + a11 * (-H / 2.0) + cy
    rec = np.zeros(B, AUGMENT_DTYPE)
    rec["m"] = np.stack([a00 / W, a01 / W, a02 / W, a10 / H, a11 / H, a12 / H], 1)
    rec["gain"] = gain
    rec["brightness"] = bright
    rec["contrast"] = contrast
    rec["saturation"] = sat
    rec["flags"] = 1 if opts.has_color else 0
    return rec


class ReaderOpts:
    """data_reader.py:72-78, plus the build's knobs: seed (shuffle + swaps), nslots (batches
    decoded ahead), pairs (an explicit pair list instead of scanning kitti_path), max_h /
    max_w (frame size bound; scanned from the PNG headers when None), augment (an AugmentOpts:
    get_batch() then augments each batch with records drawn from (seed, batch number); None:
    the plain resize)."""

    def __init__(self, kitti_path, batch_size, img_height, img_width, nworkers, seed=0,
                 nslots=3, pairs=None, max_h=None, max_w=None, augment=None):
        self.kitti_path = kitti_path
        self.batch_size = batch_size
        self.img_height = img_height
        self.img_width = img_width
        self.nworkers = nworkers
        self.seed = seed
        self.nslots = nslots
        self.pairs = pairs
        self.max_h = max_h
        self.max_w = max_w
        self.augment = augment


def _cstrings(paths: Sequence[str]):
    arr = (C.c_char_p * len(paths))()
    arr[:] = [os.fsencode(p) for p in paths]
    return arr


def png_size(path: str):
    """(h, w) from the PNG header."""
    h, w = C.c_int(), C.c_int()
    call("of_png_info", os.fsencode(path), C.byref(h), C.byref(w), None, None)
    return h.value, w.value


def imread_bgr(path: str) -> np.ndarray:
    """cv2.imread(path) (IMREAD_COLOR) on the native PNG decoder: (h, w, 3) uint8 BGR."""
    h, w = png_size(path)
    out = np.empty((h, w, 3), np.uint8)
    hh, ww = C.c_int(), C.c_int()
    call("of_png_read_bgr", os.fsencode(path), out.ctypes.data_as(C.c_void_p), out.nbytes,
         C.byref(hh), C.byref(ww))
    return out


def imwrite(path: str, img: np.ndarray, filt: int = 5, level: int = 6):
    """Write an 8-bit gray / BGR / BGRA image as PNG (cv2.imwrite's channel convention)."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    c = 1 if img.ndim == 2 else img.shape[2]
    call("of_png_write", os.fsencode(path), img.ctypes.data_as(C.c_void_p), img.shape[0],
         img.shape[1], c, filt | ((level + 1) << 8))


def split_raw(raw: np.ndarray, batch: int):
    """Decode a raw batch buffer (of_image_desc header + frames) into [(img1, img2), ...]."""
    desc = raw[:16 * 2 * batch].view(np.int64).reshape(2 * batch, 2)
    frames = []
    for k in range(2 * batch):
        off = int(desc[k, 0])
        hw = desc[k, 1:2].view(np.int32)
        h, w = int(hw[0]), int(hw[1])
        frames.append(raw[off:off + h * w * 3].reshape(h, w, 3))
    return [(frames[2 * i], frames[2 * i + 1]) for i in range(batch)]


class AsyncReader:
    """data_reader.py:81-124.  ``get_batch()`` -> (B, H, W, 6) float32 CUDA tensor, ordered on
    the current stream; ``next_raw()`` is the GPU-free hand-out (raw frames, pair ids, swap
    flags) used by the CPU tests and by ``pinned=False`` readers."""

    def __init__(self, opts: ReaderOpts, pinned: Optional[bool] = None):
        self.opts = opts
        self.data_info = opts.pairs if opts.pairs is not None else read_kitti(opts.kitti_path)
        self.nbatches = len(self.data_info) // opts.batch_size
        assert self.nbatches > 0, "fewer pairs than one batch"
        if pinned is None:
            pinned = torch.cuda.is_available()
        self.pinned = bool(pinned)
        p1 = _cstrings([p[0] for p in self.data_info])
        p2 = _cstrings([p[1] for p in self.data_info])
        max_h, max_w = opts.max_h, opts.max_w
        if max_h is None or max_w is None:
            mh, mw = C.c_int(), C.c_int()
            both = _cstrings([p for pair in self.data_info for p in pair])
            call("of_png_scan", len(both), both, max(1, opts.nworkers), C.byref(mh), C.byref(mw))
            max_h, max_w = mh.value, mw.value
        self.max_h, self.max_w = max_h, max_w
        r = C.c_void_p()
        call("of_reader_create", len(self.data_info), p1, p2, opts.batch_size, opts.nworkers,
             opts.nslots, max_h, max_w, C.c_uint64(opts.seed), int(self.pinned), C.byref(r))
        self._r = r
        self.raw_bytes = _lib.lib().of_reader_raw_bytes(r)
        self._raw_dev = None
        self._copy_stream = None
        self.last_pairs = np.zeros(opts.batch_size, np.int32)
        self.last_swapped = np.zeros(opts.batch_size, np.int32)
        self.last_augment = None          # the last batch's of_augment records (augment only)
        self._aug_dev = None
        self._batches = 0                 # get_batch() calls so far: sample_augment's batch_index

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc_val, exc_tb):
        self.close()

    def close(self):
        if self._r is not None:
            torch.cuda.synchronize() if (self.pinned and torch.cuda.is_available()) else None
            call("of_reader_destroy", self._r)
            self._r = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _meta(self):
        i32 = C.POINTER(C.c_int32)
        return self.last_pairs.ctypes.data_as(i32), self.last_swapped.ctypes.data_as(i32)

    def next_raw(self) -> np.ndarray:
        raw = np.empty(self.raw_bytes, np.uint8)
        call("of_reader_next_host", self._r, raw.ctypes.data_as(C.c_void_p), raw.nbytes,
             *self._meta())
        return raw

    def get_batch(self) -> torch.Tensor:
        assert self.pinned, "get_batch needs a reader with pinned slots (GPU present)"
        o = self.opts
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream()
            self._raw_dev = torch.empty(self.raw_bytes, dtype=torch.uint8, device="cuda")
        if o.augment is not None:
            return self._get_batch_augmented()
        compute = torch.cuda.current_stream()
        cs = self._copy_stream
        # the raw buffer is reused: order this copy after the previous preprocess (same
        # stream) -- and after the compute stream's use of nothing else (raw is private)
        with torch.cuda.stream(cs):
            out = torch.empty((o.batch_size, o.img_height, o.img_width, 6), device="cuda")
            call("of_reader_next", self._r, C.c_void_p(self._raw_dev.data_ptr()), self.raw_bytes,
                 C.c_void_p(out.data_ptr()), o.img_height, o.img_width, *self._meta(),
                 C.c_void_p(cs.cuda_stream))
        compute.wait_stream(cs)
        out.record_stream(compute)
        return out

    def _get_batch_augmented(self) -> torch.Tensor:
        """get_batch() with of_reader_next_aug: the same ordering on the copy stream, plus the
        batch's records (kept in last_augment) copied ahead of the kernel from the slot's
        pinned staging area."""
        o = self.opts
        if self._aug_dev is None:
            self._aug_dev = torch.empty(o.batch_size * AUGMENT_DTYPE.itemsize, dtype=torch.uint8,
                                        device="cuda")
        rec = sample_augment(o.augment, o.batch_size, o.img_height, o.img_width, o.seed,
                             self._batches)
        self._batches += 1
        self.last_augment = rec
        compute = torch.cuda.current_stream()
        cs = self._copy_stream
        with torch.cuda.stream(cs):
            out = torch.empty((o.batch_size, o.img_height, o.img_width, 6), device="cuda")
            call("of_reader_next_aug", self._r, C.c_void_p(self._raw_dev.data_ptr()),
                 self.raw_bytes, rec.ctypes.data_as(C.c_void_p),
                 C.c_void_p(self._aug_dev.data_ptr()), C.c_void_p(out.data_ptr()), o.img_height,
                 o.img_width, *self._meta(), C.c_void_p(cs.cuda_stream))
        compute.wait_stream(cs)
        out.record_stream(compute)
        return out


def _pack_raw(frames) -> np.ndarray:
    """[(img1_bgr_u8, img2_bgr_u8), ...] -> a raw batch buffer (of_image_desc header + frames,
    256-byte aligned: the layout the reader's slots hold)."""
    n = len(frames)
    header = -(-16 * 2 * n // 256) * 256
    offs, sizes, total = [], [], header
    for pair in frames:
        for img in pair:
            assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
            offs.append(total)
            sizes.append(img.shape[:2])
            total += -(-img.nbytes // 256) * 256
    raw = np.zeros(total, np.uint8)
    desc = raw[:16 * 2 * n].view(np.int64).reshape(2 * n, 2)
    for k, ((h, w), off) in enumerate(zip(sizes, offs)):
        desc[k, 0] = off
        desc[k, 1:2].view(np.int32)[:] = (h, w)
        img = frames[k // 2][k % 2]
        raw[off:off + img.nbytes] = np.ascontiguousarray(img).reshape(-1)
    return raw


def preprocess_frames(frames, out_h: int, out_w: int) -> torch.Tensor:
    """read_batch (data_reader.py:35-42) for frames already decoded to host memory:
    [(img1_bgr_u8, img2_bgr_u8), ...] -> (B, out_h, out_w, 6) CUDA tensor (one upload of the
    raw frames, then of_preprocess_pairs)."""
    n = len(frames)
    raw = _pack_raw(frames)
    dev = torch.from_numpy(raw).cuda()
    out = torch.empty((n, out_h, out_w, 6), device="cuda")
    call("of_preprocess_pairs", C.c_void_p(dev.data_ptr()), n, out_h, out_w,
         C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return out


def augment_frames(frames, out_h: int, out_w: int, params: np.ndarray) -> torch.Tensor:
    """preprocess_frames with of_augment_pairs: ``params`` is a (len(frames),) array of
    AUGMENT_DTYPE (sample_augment's result, or records written by hand)."""
    n = len(frames)
    params = np.ascontiguousarray(params, dtype=AUGMENT_DTYPE).reshape(-1)
    assert params.shape[0] == n, "one of_augment record per pair"
    dev = torch.from_numpy(_pack_raw(frames)).cuda()
    prm = torch.from_numpy(params.view(np.uint8)).cuda()
    out = torch.empty((n, out_h, out_w, 6), device="cuda")
    call("of_augment_pairs", C.c_void_p(dev.data_ptr()), n, out_h, out_w,
         C.c_void_p(prm.data_ptr()), C.c_void_p(out.data_ptr()),
         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return out


def read_item(item_info, opts: ReaderOpts, swap: Optional[bool] = None):
    """data_reader.py:45-64 for one pair: (image1, image2), each (H, W, 3) float32 on the GPU.
    swap=None draws the p=0.5 order swap like the reference."""
    if swap is None:
        swap = bool(np.random.rand() >= 0.5)
    path1, path2 = (item_info[1], item_info[0]) if swap else (item_info[0], item_info[1])
    batch = preprocess_frames([(imread_bgr(path1), imread_bgr(path2))], opts.img_height,
                              opts.img_width)
    return batch[0, :, :, :3], batch[0, :, :, 3:]


def read_batch(batch_info, opts: ReaderOpts, swaps: Optional[Sequence[bool]] = None):
    """data_reader.py:35-42 synchronously: (B, H, W, 6) float32 on the GPU."""
    frames = []
    for i, item in enumerate(batch_info):
        sw = bool(np.random.rand() >= 0.5) if swaps is None else bool(swaps[i])
        a, b = (item[1], item[0]) if sw else (item[0], item[1])
        frames.append((imread_bgr(a), imread_bgr(b)))
    out = torch.zeros((opts.batch_size, opts.img_height, opts.img_width, 6), device="cuda")
    out[:len(frames)] = preprocess_frames(frames, opts.img_height, opts.img_width)
    return out
