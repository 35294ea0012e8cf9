"""Mirror of the reference ``train.py`` driver (train.py:1-88).

``train_step(batch_imgs, step_count)`` keeps the reference's shape (train.py:47-61): forward
through the flow net, the photometric loss, gradients of the trainable weights, one Keras-Adam
update; returns ``(loss_value, flows)``.  Data: ``--kitti PATH`` reads KITTI raw pairs
through the native AsyncReader (data_reader.py; batches land in HBM already resized and
normalised), otherwise synthetic pairs with the reference value contract (data.py).
``--display-dir`` writes the every-10-batches display_training pictures (train.py:80-81) as
PNGs.  No TensorBoard writer (a JSONL step log instead).  Data parallelism (one process per
GPU, RCCL all-reduce of gradient buckets overlapped with the backward) is build-added; with
KITTI each rank reads its own seeded shuffle.  ``--augment`` (KITTI only) switches on the
seeded GPU augmentation of data_reader.AugmentOpts: random zoom / crop, flip, colour jitter.
``--kitti-flow ROOT`` reads the labelled frames of a KITTI 2015 flow tree instead and, with
``--supervised-weight`` > 0, fine-tunes on their sparse ground truth (evaluate.KittiFlowReader;
``--kitti-flow-holdout K`` keeps every K-th frame for evaluation); ``--kitti-flow-augment`` /
``--kitti-flow-aug-*`` augment those frames and carry their ground truth along (of_gt_augment).
``--selfsup-weight W`` > 0 adds augmentation self-supervision (the teacher's flow on the batch
as read is the target on the batch moved through the ``--augment`` / ``--aug-*`` transform, on
the device, so it also runs without ``--kitti``; ``--selfsup-start-epoch E`` starts it later;
with ``--occlusion range`` the teacher's weight is the soft range-map mask, carried bilinearly).
``--clip-norm C`` / ``--skip-nonfinite`` / ``--log-grad-norm`` switch on KerasAdam's global-norm
clipping, its non-finite update guard and the per-step gradient norm in the step log.

Run:  python -m optical_flow_amd.train --height 384 --width 512 --batch 8 --steps 20
      python -m optical_flow_amd.train --kitti /data/kitti_raw --epochs 20
      python -m optical_flow_amd.train --kitti /data/kitti_raw --epochs 20 --augment
      python -m optical_flow_amd.train --kitti-flow /data/kitti_flow --warp-convention image \\
          --photometric-weight 0 --supervised-weight 1 --supervised-q 0.4 \\
          --kitti-flow-holdout 5 --pretrained ckpt/flow_net_19/weights --kitti-flow-augment
      python -m optical_flow_amd.train --kitti /data/kitti_raw --warp-convention image \\
          --occlusion fb --census-weight 1 --selfsup-weight 0.3 --selfsup-start-epoch 5 --augment
"""
from __future__ import annotations

import argparse
import contextlib
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np
import torch

from . import ops
from ._lib import call, lib
from .data import synthetic_batch
from .dist import GradBucketReducer, init_from_env
from .loss import LossLayer
from .model import FlowNet, build_flow_net


class KerasAdam:
    """tf.keras.optimizers.Adam (train.py:34): beta_1 0.9, beta_2 0.999, epsilon 1e-7,
    ResourceApplyAdam update with lr_t = lr*sqrt(1-b2^t)/(1-b1^t) (P13).  Two launches over
    the model's parameter arena: the step counter t and lr_t live in device memory
    (of_adam_keras_dev), so the same update also runs inside a captured HIP graph
    (Trainer.graphed).  ``learning_rate`` may be set between steps (train.py:69-70).

    Build-added, all off by default (then ``apply_gradients`` is the one of_adam_keras_dev
    call):

    global_clipnorm: Keras's argument of that name, tf.clip_by_global_norm over all gradients:
        with norm = the L2 norm of the whole (averaged) gradient, every gradient is multiplied
        by global_clipnorm / max(norm, global_clipnorm).  A step whose norm is at or under the
        threshold is bitwise the unclipped step.  As in TensorFlow, a non-finite norm (one inf
        or NaN gradient element) makes the multiplier NaN and so every parameter NaN, unless
        skip_nonfinite is set.  Settable between eager steps, like learning_rate.
    skip_nonfinite: a step whose gradient norm is inf or NaN is dropped on the device:
        parameters, both moments and the step counter stay bitwise as they were, and
        ``skipped_updates`` counts it.
    track_grad_norm: only record the norm (``last_grad_norm``).

    With any of them on, the update is two calls, of_grad_sumsq and of_adam_keras_dev_clip: the
    norm, the multiplier and the skip decision are formed on the device, with no host
    read-back and no allocation after construction, so the update stays capturable."""

    def __init__(self, store, learning_rate=1e-4, beta_1=0.9, beta_2=0.999, epsilon=1e-7,
                 global_clipnorm=None, skip_nonfinite=False, track_grad_norm=False):
        self.store = store
        self.beta_1, self.beta_2, self.epsilon = beta_1, beta_2, epsilon
        dev = store.arena.device
        self.m = torch.zeros_like(store.arena)
        self.v = torch.zeros_like(store.arena)
        self._sched = torch.zeros(2, device=dev)              # [lr, lr_t of the last step]
        self._iter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.learning_rate = learning_rate
        self.global_clipnorm = global_clipnorm
        self.skip_nonfinite = bool(skip_nonfinite)
        self.track_grad_norm = bool(track_grad_norm)
        self._partials = self._state = None
        if self._clip_path():
            self._alloc_clip()

    @staticmethod
    def check_global_clipnorm(value):
        """None, or the positive finite float of ``global_clipnorm``; ValueError otherwise."""
        if value is None:
            return None
        c = float(value)
        if not (math.isfinite(c) and c > 0.0):
            raise ValueError("global_clipnorm must be a positive finite number, got %r" % (value,))
        return c

    @property
    def global_clipnorm(self):
        return self._clipnorm

    @global_clipnorm.setter
    def global_clipnorm(self, value):
        self._clipnorm = self.check_global_clipnorm(value)

    def _clip_path(self):
        return self._clipnorm is not None or self.skip_nonfinite or self.track_grad_norm

    def _alloc_clip(self):
        dev = self.store.arena.device
        n = lib().of_grad_sumsq_partials(self.store.numel)
        self._partials = torch.zeros(n, dtype=torch.float64, device=dev)
        # the of_adam_keras_dev_clip state block (include/oflow.h): norm f64, norm f32, mult f32,
        # skip i32, skipped_total i32
        self._state = torch.zeros(lib().of_adam_clip_state_bytes() // 8, dtype=torch.float64,
                                  device=dev)

    def _clip_state(self):
        if self._state is None:
            raise RuntimeError("KerasAdam was built without global_clipnorm, skip_nonfinite or "
                               "track_grad_norm: no gradient norm is computed")
        return self._state

    @property
    def last_grad_norm(self):
        """The global gradient norm of the last apply_gradients (of the averaged gradient under
        data parallelism; inf or NaN for a non-finite gradient): a 0-dim float64 device tensor,
        a view into the state block that every later step overwrites -- no sync until read."""
        return self._clip_state()[0]

    @property
    def skipped_updates(self):
        """Updates dropped by skip_nonfinite so far (device counter, read with a sync)."""
        return int(self._clip_state().view(torch.int32)[5].item())

    @property
    def learning_rate(self):
        return self._lr

    @learning_rate.setter
    def learning_rate(self, lr):
        self._lr = float(lr)
        self._sched[0].fill_(self._lr)

    @property
    def iterations(self):
        """Updates applied so far (device counter: replays of a captured step count too)."""
        return int(self._iter.item())

    def apply_gradients(self, grad_scale: float = 1.0):
        s = self.store
        if self._clip_path():
            if self._state is None:      # switched on after construction (eager steps only)
                self._alloc_clip()
            stream = ops._stream()
            call("of_grad_sumsq", C.c_void_p(s.grad_arena.data_ptr()), s.numel,
                 C.c_void_p(self._partials.data_ptr()), stream)
            call("of_adam_keras_dev_clip", C.c_void_p(s.arena.data_ptr()),
                 C.c_void_p(s.grad_arena.data_ptr()), C.c_void_p(self.m.data_ptr()),
                 C.c_void_p(self.v.data_ptr()), s.numel, C.c_void_p(self._sched.data_ptr()),
                 C.c_void_p(self._iter.data_ptr()), self.beta_1, self.beta_2, self.epsilon,
                 grad_scale, C.c_void_p(self._partials.data_ptr()), self._partials.numel(),
                 self._clipnorm or 0.0, int(self.skip_nonfinite),
                 C.c_void_p(self._state.data_ptr()), stream)
        else:
            call("of_adam_keras_dev", C.c_void_p(s.arena.data_ptr()),
                 C.c_void_p(s.grad_arena.data_ptr()), C.c_void_p(self.m.data_ptr()),
                 C.c_void_p(self.v.data_ptr()), s.numel, C.c_void_p(self._sched.data_ptr()),
                 C.c_void_p(self._iter.data_ptr()), self.beta_1, self.beta_2, self.epsilon,
                 grad_scale, ops._stream())
        s.version += 1       # packed conv weights are refreshed lazily on next use
        if getattr(s, "bn_guard", None) is not None:
            s.bn_guard.after_update(self._lr)


def check_warp_conventions(flow_net, loss_layer):
    """The net's warp and the loss layer's must sample one convention: training across two is
    never meant (the loss would score flows the net's warps read differently).  An object
    without the attribute (TwoLayerHead, a custom loss) counts as "reference"."""
    net_cv = getattr(flow_net, "warp_convention", "reference")
    loss_cv = getattr(loss_layer, "warp_convention", "reference")
    if net_cv != loss_cv:
        raise ValueError("the net warps in the %r convention and the loss layer in %r: "
                         "build both with the same warp_convention" % (net_cv, loss_cv))
    return net_cv


def check_selfsup(flow_net, loss_layer, selfsup):
    """Trainer's self-supervision arguments: the AugmentOpts and a loss layer with
    ``selfsup_weight`` > 0 need each other, and the teacher pass must not move BatchNorm's
    moving statistics a second time.  ValueError otherwise."""
    w = getattr(loss_layer, "selfsup_weight", 0.0)
    if selfsup is None:
        if w > 0:
            raise ValueError("the loss layer has selfsup_weight > 0: the trainer needs the "
                             "augmentation to self-supervise with (selfsup=AugmentOpts(...))")
        return
    from .data_reader import AugmentOpts
    if not isinstance(selfsup, AugmentOpts):
        raise ValueError("selfsup must be a data_reader.AugmentOpts, got %r" % (selfsup,))
    if not w > 0:
        raise ValueError("selfsup given, but the loss layer's selfsup_weight is 0")
    if getattr(flow_net, "bn_mode", "inference") == "training":
        raise ValueError("self-supervision runs a teacher pass before the step: with "
                         "bn_mode='training' it would update the moving statistics a second "
                         "time; use bn_mode='inference'")


class Trainer:
    """Holds the model, optimizer, loss and (optional) DP reducer; ``train_step`` is the
    hot loop body of train.py:72-82."""

    def __init__(self, flow_net: FlowNet, optimizer: KerasAdam = None, loss_layer=None,
                 data_parallel: bool = None, comm=None, selfsup=None, selfsup_seed=0):
        """data_parallel: sum the gradients over ranks before Adam (default: when a
        torch.distributed group of > 1 ranks exists).  comm: a communicator (comm.py), or
        "rccl" / "torch" to create one; default "rccl" for a GPU model (the C-ABI RCCL
        communicator over all ranks of the default group), "torch" otherwise.

        selfsup: a data_reader.AugmentOpts switches on augmentation self-supervision, for a
        loss layer with ``selfsup_weight`` > 0 (and such a layer needs it): every step first
        runs the net without gradients on the batch as given (the teacher), draws one
        augmentation record per pair from (selfsup_seed, step number), and trains on the
        augmented batch with the teacher's flow, carried through the same records, as the
        target of the finest flow (train_step; DESIGN.md "Self-supervision")."""
        self.flow_net = flow_net
        self.optimizer = optimizer or KerasAdam(flow_net.store)
        self.loss_layer = loss_layer or LossLayer(
            warp_convention=getattr(flow_net, "warp_convention", "reference"))
        check_warp_conventions(flow_net, self.loss_layer)
        check_selfsup(flow_net, self.loss_layer, selfsup)
        self.selfsup = selfsup
        self.selfsup_seed = int(selfsup_seed)
        self.selfsup_enabled = selfsup is not None
        self.last_selfsup = None
        self._selfsup_step = 0
        if data_parallel is None:
            data_parallel = comm is not None or (torch.distributed.is_initialized() and
                                                 torch.distributed.get_world_size() > 1)
        self.reducer = None
        if data_parallel:
            if comm is None or isinstance(comm, str):
                from .comm import make_comm
                dist = torch.distributed
                rank, world = ((dist.get_rank(), dist.get_world_size())
                               if dist.is_initialized() else (0, 1))
                kind = comm or os.environ.get("OFLOW_DP_COMM") or (
                    "rccl" if flow_net.store.arena.is_cuda else "torch")
                comm = make_comm(kind, rank, world)
            self.reducer = GradBucketReducer(flow_net.store, comm=comm)

    def teacher_pass(self, batch_imgs):
        """The self-supervision teacher: the net's flows on ``batch_imgs`` without gradients
        (on the doubled batch under occlusion="fb" or "range") and the level-0 occlusion mask
        of the first B images (None under occlusion="none"; under "range" the soft weight,
        which transform_flow carries bilinearly like any mask).  Weights, gradients, buffers
        and ``store.version`` stay untouched.  Returns (finest flow (B, h, w, 2), mask)."""
        nb = batch_imgs.shape[0]
        occ = getattr(self.loss_layer, "occlusion", "none")
        with torch.no_grad():
            x = batch_imgs
            if ops.needs_swapped_pairs(occ):
                x = torch.cat([x, torch.cat([x[..., 3:], x[..., :3]], -1)], 0)
            flows = self.flow_net(x)
            mask = None
            if occ != "none":
                mask = ops.occlusion_masks(flows, occ, self.loss_layer.occlusion_alpha1,
                                           self.loss_layer.occlusion_alpha2,
                                           self.loss_layer.warp_convention)[0][:nb]
            return flows[0][:nb].contiguous(), mask

    def _selfsup_inputs(self, batch_imgs, records):
        """Steps 1 and 2 of a self-supervised step: (augmented batch, (target, weight))."""
        from .data_reader import sample_augment
        nb, H, W = batch_imgs.shape[:3]
        teacher, mask = self.teacher_pass(batch_imgs)
        if records is None:
            records = sample_augment(self.selfsup, nb, H, W, self.selfsup_seed,
                                     self._selfsup_step)
        self._selfsup_step += 1
        rec = ops._records_dev(records, nb, batch_imgs.device)
        student = ops.augment_batch(batch_imgs, rec)
        target, weight = ops.transform_flow(teacher, rec, (H, W), mask)
        self.last_selfsup = {"batch": student, "target": target, "weight": weight,
                             "records": rec}
        return student, (target, weight)

    def train_step(self, batch_imgs, step_count=0, gt=None, selfsup_records=None):
        """``gt``: the batch's KITTI flow ground truth for a loss layer with
        ``supervised_weight`` > 0 (what LossLayer's call takes); None otherwise.
        ``selfsup_records``: with self-supervision on, this step's of_augment records (an
        AUGMENT_DTYPE array or a CUDA uint8 tensor) in place of the seeded draw.  A
        self-supervised step trains on the augmented batch and returns its flows;
        ``last_selfsup`` then holds that batch, the target, the weight and the records.
        ``selfsup_enabled = False`` makes the step the plain one."""
        selfsup = None
        if self.selfsup is not None and self.selfsup_enabled:
            batch_imgs, selfsup = self._selfsup_inputs(batch_imgs, selfsup_records)
        elif selfsup_records is not None:
            raise ValueError("selfsup_records given, but self-supervision is off")
        store = self.flow_net.store
        store.zero_grad()
        if self.reducer is not None:
            self.reducer.begin()
        nb = batch_imgs.shape[0]
        if ops.needs_swapped_pairs(getattr(self.loss_layer, "occlusion", "none")):
            # forward-backward check, range map: the net also sees every pair with its images
            # exchanged ([batch ; swapped], device-only ops: the step still captures); the loss
            # is the mean over both directions
            batch_imgs = torch.cat([batch_imgs,
                                    torch.cat([batch_imgs[..., 3:], batch_imgs[..., :3]], -1)], 0)
        flows = self.flow_net(batch_imgs)
        if selfsup is not None or self.selfsup is not None:
            loss_value = self._selfsup_loss(batch_imgs, flows, gt, selfsup)
        elif gt is not None:
            loss_value = self.loss_layer(batch_imgs, flows, gt=gt)
        else:                           # as it always was (a custom loss takes two arguments)
            loss_value = self.loss_layer(batch_imgs, flows)
        loss_value.backward()
        scale = 1.0
        if self.reducer is not None:
            # bn_mode "training": the moving statistics this step updated on every rank are
            # averaged over the ranks (dist.GradBucketReducer.finish), so replicas stay equal
            bufs = store.buffers if getattr(self.flow_net, "bn_mode", "") == "training" else None
            scale = self.reducer.finish(buffers=bufs)
        self.optimizer.apply_gradients(grad_scale=scale)
        # "fb", "range": the caller sees the forward flows of the batch it passed
        return loss_value.detach(), [f.detach()[:nb] for f in flows]

    def _selfsup_loss(self, batch_imgs, flows, gt, selfsup):
        """The loss of a trainer built with self-supervision.  While it is switched off
        (``selfsup_enabled`` False) the layer is called without a target and its
        self-supervision term contributes nothing."""
        layer = self.loss_layer
        kw = {"gt": gt} if gt is not None else {}
        if selfsup is not None:
            return layer(batch_imgs, flows, selfsup=selfsup, **kw)
        w, layer.selfsup_weight = layer.selfsup_weight, 0.0
        try:
            return layer(batch_imgs, flows, **kw)
        finally:
            layer.selfsup_weight = w

    def graphed(self, batch_imgs, warmup: int = 2, capture_ctx=None):
        """The step captured once as a HIP graph over a static input batch (train.py:47-48
        traces train_step once as a tf.function; this is the MI355X counterpart): returns a
        GraphedStep whose call copies nothing and replays every kernel of forward, loss,
        backward, bucket all-reduce (RCCL) and Adam with no host work per launch.
        ``warmup`` eager steps run first (they train, like any step)."""
        return GraphedStep(self, batch_imgs, warmup, capture_ctx)


# The captured step replays on a HIGH-priority stream of its own (torch.cuda.Stream(priority=-1),
# ordered after and before the caller's stream).  The HIP runtime inside the torch wheel (ROCm
# 7.0.2 libamdhip64, which liboflow binds to in a torch process) assigns a graph executor's
# parallel streams at its first launch by skipping those on the launch stream's hardware queue,
# without bounds: when one of them shares that queue it reads past the end of its stream list
# and segfaults in hipGraphLaunch (native backtrace, and the subset that
# crashed passing with this change).  Which queue a stream gets depends on every stream the
# process made before (RCCL's included); high-priority streams take their queues from a set of
# their own, so the normal-priority parallel streams never share the launch stream's.
# OFLOW_GRAPH_REPLAY_PRIO overrides the priority ("none": replay on the caller's stream).
_RP = os.environ.get("OFLOW_GRAPH_REPLAY_PRIO", "-1")
REPLAY_PRIO = None if _RP == "none" else int(_RP)


class GraphedStep:
    """A captured Trainer.train_step.  ``batch`` is the static input: write the next batch
    into it (``load``) before calling.  Returns the static (loss, flows) tensors, overwritten
    by every replay.

    Every host argument of the step is baked into the capture, the optimizer's
    ``global_clipnorm``, ``skip_nonfinite`` and ``track_grad_norm`` among them: set them before
    capturing (the learning rate is the exception, it lives in device memory).  The clip and
    skip decisions themselves are taken on the device in every replay; ``last_grad_norm`` and
    ``skipped_updates`` read the replays' results."""

    def __init__(self, trainer: "Trainer", batch_imgs, warmup: int = 2, capture_ctx=None):
        """capture_ctx: optional context-manager factory entered around the capture only (the
        bench arms its kernel timing there)."""
        if trainer.reducer is not None and getattr(trainer.reducer.comm, "kind", "") != "rccl":
            raise RuntimeError("graph capture needs the RCCL communicator (gloo collectives "
                               "cannot be captured)")
        if getattr(trainer, "selfsup", None) is not None:
            raise RuntimeError("graph capture does not take a self-supervised trainer "
                               "(selfsup=...): the teacher pass and the per-step records are "
                               "not captured; run train_step(batch) eagerly")
        if getattr(trainer.loss_layer, "supervised_weight", 0.0) != 0.0:
            raise RuntimeError("graph capture does not take a supervised loss layer "
                               "(supervised_weight > 0): the ground-truth buffer changes size "
                               "from batch to batch; run train_step(batch, gt=...) eagerly")
        self.trainer = trainer
        self.batch = batch_imgs
        cur = torch.cuda.current_stream()
        s = torch.cuda.Stream()
        s.wait_stream(cur)
        with torch.cuda.stream(s):                   # warm-up off the default stream (torch
            for i in range(warmup):                  # capture rule), creates the side streams
                trainer.train_step(batch_imgs, i)
        cur.wait_stream(s)
        self.captures = 0
        self._rs = None
        self._capture(capture_ctx)

    def _capture(self, capture_ctx=None):
        self.graph = torch.cuda.CUDAGraph()
        with capture_ctx() if capture_ctx is not None else contextlib.nullcontext():
            with torch.cuda.graph(self.graph):
                self.loss, self.flows = self.trainer.train_step(self.batch)
        self.captures += 1

    def load(self, batch_imgs):
        self.batch.copy_(batch_imgs, non_blocking=True)

    def __call__(self, batch_imgs=None, step_count=0):
        """One replay.  The BN gamma guard (ops.BNZGuard) is driven from here: the captured
        step bakes in which BN layers store z, so every BNZGuard.EVERY replays the guard's
        min |gamma| check is launched after the replay (read back asynchronously), and when a
        check flags a new layer the step is captured again before the next replay, so that
        layer's backward reads the stored z instead of recovering it through gamma ~ 0."""
        store = self.trainer.flow_net.store
        guard = store.bn_guard
        if guard is not None and guard.layers:
            before = len(guard.flagged)
            guard.poll()
            if len(guard.flagged) != before:
                torch.cuda.synchronize()
                self._capture()
        if batch_imgs is not None and batch_imgs.data_ptr() != self.batch.data_ptr():
            self.load(batch_imgs)
        if REPLAY_PRIO is None:
            self.graph.replay()
        else:
            # on a stream of its own priority (REPLAY_PRIO: the hipGraphLaunch fault)
            if self._rs is None:
                self._rs = torch.cuda.Stream(priority=REPLAY_PRIO)
            cur = torch.cuda.current_stream()
            self._rs.wait_stream(cur)
            with torch.cuda.stream(self._rs):
                self.graph.replay()
            cur.wait_stream(self._rs)
        store.version += 1
        red = self.trainer.reducer
        if red is not None:
            # the captured step's collectives are not watched inside the capture (an event
            # recorded there would only complete in a replay): bound this replay's instead
            comm = red.comm
            if getattr(comm, "watchdog", None) is not None:
                comm.watch_stream(torch.cuda.current_stream())
                comm.watchdog.check()
        if guard is not None:
            guard.after_update(self.trainer.optimizer.learning_rate)
        return self.loss, self.flows


# --augment: zoom 1-1.3 with translation, hflip 0.5, brightness +-0.1, contrast, saturation
# 0.8-1.2, colour gain 0.9-1.1 (no rotation)
AUGMENT_PRESET = dict(zoom=(1.0, 1.3), translate=True, hflip_prob=0.5, rotate_deg=0.0,
                      brightness=0.1, contrast=(0.8, 1.2), saturation=(0.8, 1.2),
                      color_gain=(0.9, 1.1))


def augment_from_args(args):
    """The AugmentOpts of the command line: None without any augmentation flag; --augment is
    AUGMENT_PRESET; each --aug-* override replaces one field of the preset, or of the identity
    when --augment is not given.  ValueError (AugmentOpts) for a bad value."""
    from .data_reader import AugmentOpts
    over = {}
    if args.aug_zoom_max is not None:
        over["zoom"] = (1.0, args.aug_zoom_max)
    if args.aug_hflip is not None:
        over["hflip_prob"] = args.aug_hflip
    if args.aug_rotate is not None:
        over["rotate_deg"] = args.aug_rotate
    if args.aug_brightness is not None:
        over["brightness"] = args.aug_brightness
    for name, key in (("aug_contrast", "contrast"), ("aug_saturation", "saturation"),
                      ("aug_color_gain", "color_gain")):
        a = getattr(args, name)
        if a is not None:
            over[key] = (1.0 - a, 1.0 + a)
    if not args.augment and not over:
        return None
    kw = dict(AUGMENT_PRESET) if args.augment else {}
    kw.update(over)
    return AugmentOpts(**kw)


def kitti_flow_augment_from_args(args):
    """The AugmentOpts of --kitti-flow-augment / --kitti-flow-aug-*, which augment the labelled
    frames together with their ground truth: None without any of them; --kitti-flow-augment is
    AUGMENT_PRESET; each override replaces one field of the preset, or of the identity without
    it.  ValueError (AugmentOpts) for a bad value."""
    from .data_reader import AugmentOpts
    over = {}
    if args.kitti_flow_aug_zoom_max is not None:
        over["zoom"] = (1.0, args.kitti_flow_aug_zoom_max)
    if args.kitti_flow_aug_hflip is not None:
        over["hflip_prob"] = args.kitti_flow_aug_hflip
    if args.kitti_flow_aug_rotate is not None:
        over["rotate_deg"] = args.kitti_flow_aug_rotate
    if not args.kitti_flow_augment and not over:
        return None
    kw = dict(AUGMENT_PRESET) if args.kitti_flow_augment else {}
    kw.update(over)
    return AugmentOpts(**kw)


def check_kitti_flow_augment_args(args, label_augment):
    """--kitti-flow-augment / --kitti-flow-aug-* (``label_augment``: their AugmentOpts, or None)
    need --kitti-flow, whose frames they augment, and --warp-convention image: the ground truth
    they carry is an image displacement.  ValueError otherwise (main turns it into a parser
    error)."""
    if label_augment is None:
        return
    if not args.kitti_flow:
        raise ValueError("--kitti-flow-augment / --kitti-flow-aug-* need --kitti-flow: they "
                         "augment its labelled frames and ground truth")
    if args.warp_convention != "image":
        raise ValueError("--kitti-flow-augment / --kitti-flow-aug-* need --warp-convention image: "
                         "the ground truth they carry is an image displacement")


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--height", type=int, default=192)       # train.py:15
    ap.add_argument("--width", type=int, default=640)        # train.py:16
    ap.add_argument("--batch", type=int, default=4)          # train.py:20
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10, help="batches per epoch")
    ap.add_argument("--lr", type=float, default=1e-4)        # train.py:34
    ap.add_argument("--lr-drop-epoch", type=int, default=15)  # train.py:69-70
    ap.add_argument("--pretrained", default=None)
    ap.add_argument("--save-dir", default=None)
    ap.add_argument("--log", default=None, help="JSONL step log")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--kitti", default=None, help="KITTI raw root (train.py:20)")
    ap.add_argument("--nworkers", type=int, default=6)      # train.py:22
    ap.add_argument("--display-dir", default=None, help="PNG flow pictures every 10 batches")
    ap.add_argument("--smoothness-weight", type=float, default=0.0,
                    help="weight of the edge-aware flow smoothness term (0: the reference loss)")
    ap.add_argument("--edge-alpha", type=float, default=0.0,
                    help="edge sensitivity of the smoothness term (0: unweighted)")
    ap.add_argument("--smoothness-order", type=int, default=1, choices=(1, 2),
                    help="the smoothness term penalises the flow's first (1) or second (2) "
                         "differences; 2 leaves an affine flow free")
    ap.add_argument("--census-weight", type=float, default=0.0,
                    help="weight of the soft ternary census data term (0: off)")
    ap.add_argument("--census-radius", type=int, default=3, choices=(1, 2, 3),
                    help="census window radius r, a (2r+1) x (2r+1) window")
    ap.add_argument("--photometric-weight", type=float, default=1.0,
                    help="weight of the photometric L1 term (0 with --census-weight: census only)")
    ap.add_argument("--ssim-weight", type=float, default=0.0,
                    help="weight of the 3x3 SSIM data term (0: off); the usual mix is "
                         "--photometric-weight 0.15 --ssim-weight 0.85")
    ap.add_argument("--clip-norm", type=float, default=None, metavar="C",
                    help="clip the gradients to global L2 norm C (Keras global_clipnorm)")
    ap.add_argument("--skip-nonfinite", action="store_true",
                    help="drop an update whose gradient norm is inf or NaN")
    ap.add_argument("--log-grad-norm", action="store_true",
                    help="record the global gradient norm of every step in the step log")
    ap.add_argument("--warp-convention", default="reference", choices=("reference", "image"),
                    help="the grid every warp adds the flow to: the reference's transposed grid "
                         "(default) or image coordinates (flow = (x, y) displacement)")
    ap.add_argument("--occlusion", default="none", choices=("none", "border", "fb", "range"),
                    help="mask the data terms where the sample leaves the frame (border) or "
                         "also fails the forward-backward check (fb: every step runs the "
                         "pairs both ways), or weigh them by the soft range map of the "
                         "backward flow (range: both ways too, no thresholds, the alphas play "
                         "no part); needs --warp-convention image")
    ap.add_argument("--occ-alpha1", type=float, default=0.01,
                    help="relative tolerance of the forward-backward check")
    ap.add_argument("--occ-alpha2", type=float, default=0.5,
                    help="absolute tolerance of the forward-backward check, in squared "
                         "full-resolution pixels")
    ap.add_argument("--kitti-flow", default=None, metavar="ROOT",
                    help="train on the labelled frames of a KITTI 2015 flow tree (supervised "
                         "fine-tuning; excludes --kitti, no augmentation)")
    ap.add_argument("--kitti-flow-holdout", type=int, default=0, metavar="K",
                    help="with --kitti-flow: keep every K-th frame out of training and evaluate "
                         "on those after every --eval-every epochs and at the end")
    ap.add_argument("--supervised-weight", type=float, default=0.0,
                    help="weight of the supervised end-point-error term against the ground "
                         "truth (0: off); needs --kitti-flow and --warp-convention image")
    ap.add_argument("--supervised-q", type=float, default=1.0,
                    help="exponent of the supervised penalty (|e|^2 + eps^2)^(q/2); 0.4 is the "
                         "robust fine-tuning penalty of the PWC-Net family")
    ap.add_argument("--supervised-eps", type=float, default=0.01,
                    help="eps of the supervised penalty, in native pixels")
    ap.add_argument("--selfsup-weight", type=float, default=0.0, metavar="W",
                    help="weight of the augmentation self-supervision term (0: off): the net's "
                         "flow on the batch as read, carried through the --augment / --aug-* "
                         "transform, is the target of its flow on the transformed batch; needs "
                         "--warp-convention image")
    ap.add_argument("--selfsup-q", type=float, default=0.4,
                    help="exponent of the self-supervision penalty (|e|^2 + eps^2)^(q/2)")
    ap.add_argument("--selfsup-eps", type=float, default=0.01,
                    help="eps of the self-supervision penalty, in cells of the finest flow")
    ap.add_argument("--selfsup-start-epoch", type=int, default=0, metavar="E",
                    help="epochs before E train without the self-supervision term")
    ap.add_argument("--eval-kitti-flow", default=None, metavar="ROOT",
                    help="KITTI 2015 flow root: EPE and Fl-all against its ground truth after "
                         "every --eval-every epochs and at the end (needs --warp-convention image)")
    ap.add_argument("--eval-every", type=int, default=1, metavar="N",
                    help="epochs between evaluations (with --eval-kitti-flow)")
    g = ap.add_argument_group(
        "augmentation (with --kitti, or with --selfsup-weight)", "seeded by --seed; both images "
        "of a pair get the same draw; an --aug-* flag without --augment starts from no "
        "augmentation; with --selfsup-weight the flags set the self-supervision transform, which "
        "runs on the device, and the reader stays un-augmented")
    g.add_argument("--augment", action="store_true",
                   help="preset: zoom 1-1.3 with random crop position, horizontal flip p=0.5, "
                        "brightness +-0.1, contrast 0.8-1.2, saturation 0.8-1.2, per-channel "
                        "colour gain 0.9-1.1")
    g.add_argument("--aug-zoom-max", type=float, default=None, metavar="Z",
                   help="zoom uniform in [1, Z]; the crop is 1/zoom of the frame per axis")
    g.add_argument("--aug-hflip", type=float, default=None, metavar="P",
                   help="probability of a horizontal flip")
    g.add_argument("--aug-rotate", type=float, default=None, metavar="DEG",
                   help="rotation uniform in +-DEG about the image centre (preset: 0)")
    g.add_argument("--aug-brightness", type=float, default=None, metavar="D",
                   help="brightness delta uniform in +-D (pixel values in [0, 1])")
    g.add_argument("--aug-contrast", type=float, default=None, metavar="A",
                   help="contrast factor uniform in [1-A, 1+A]")
    g.add_argument("--aug-saturation", type=float, default=None, metavar="A",
                   help="saturation factor uniform in [1-A, 1+A]")
    g.add_argument("--aug-color-gain", type=float, default=None, metavar="A",
                   help="per-channel gain uniform in [1-A, 1+A]")
    g = ap.add_argument_group(
        "augmentation of the labelled frames (with --kitti-flow and --warp-convention image)",
        "seeded by --seed; a frame's two images and its ground-truth map get the same draw, the "
        "map by a nearest-pixel gather with its vectors mapped through the crop; a "
        "--kitti-flow-aug-* flag without --kitti-flow-augment starts from no augmentation; "
        "held-out and evaluation frames are never augmented")
    g.add_argument("--kitti-flow-augment", action="store_true",
                   help="the --augment preset on the labelled frames and their ground truth")
    g.add_argument("--kitti-flow-aug-zoom-max", type=float, default=None, metavar="Z",
                   help="zoom uniform in [1, Z]; the crop is 1/zoom of the frame per axis")
    g.add_argument("--kitti-flow-aug-hflip", type=float, default=None, metavar="P",
                   help="probability of a horizontal flip")
    g.add_argument("--kitti-flow-aug-rotate", type=float, default=None, metavar="DEG",
                   help="rotation uniform in +-DEG about the image centre (preset: 0)")
    return ap


def check_eval_args(args):
    """--eval-kitti-flow measures image displacements, so it needs --warp-convention image;
    --eval-every counts epochs.  ValueError otherwise (main turns it into a parser error)."""
    if args.eval_kitti_flow is None:
        return
    if args.warp_convention != "image":
        raise ValueError("--eval-kitti-flow needs --warp-convention image: a reference-convention "
                         "flow is not an image displacement, its error against ground truth "
                         "means nothing")
    if args.eval_every < 1:
        raise ValueError("--eval-every must be >= 1, got %d" % args.eval_every)


def check_supervised_args(args):
    """--kitti-flow excludes --kitti; --supervised-weight > 0 needs --kitti-flow (the labelled
    frames) and --warp-convention image; --kitti-flow-holdout needs --kitti-flow and is 0 (off)
    or >= 2.  ValueError otherwise (main turns it into a parser error)."""
    if args.kitti_flow is not None and args.kitti is not None:
        raise ValueError("--kitti-flow and --kitti exclude each other: one run reads one data set")
    if args.supervised_weight < 0:
        raise ValueError("--supervised-weight must be >= 0, got %r" % (args.supervised_weight,))
    if args.supervised_weight > 0:
        if args.kitti_flow is None:
            raise ValueError("--supervised-weight > 0 needs --kitti-flow: only its frames carry "
                             "ground truth")
        if args.warp_convention != "image":
            raise ValueError("--supervised-weight > 0 needs --warp-convention image: a "
                             "reference-convention flow is not an image displacement")
    if args.kitti_flow_holdout:
        if args.kitti_flow is None:
            raise ValueError("--kitti-flow-holdout needs --kitti-flow")
        if args.kitti_flow_holdout < 2:
            raise ValueError("--kitti-flow-holdout must be >= 2, got %d" % args.kitti_flow_holdout)
        if args.warp_convention != "image":
            raise ValueError("--kitti-flow-holdout evaluates image displacements: it needs "
                             "--warp-convention image")
        if args.eval_every < 1:
            raise ValueError("--eval-every must be >= 1, got %d" % args.eval_every)


def check_augment_args(args, augment):
    """Where the augmentation flags (``augment``: their AugmentOpts, or None) apply: never with
    --kitti-flow; with --kitti, where the reader augments; and with --selfsup-weight > 0, where
    they set the self-supervision transform, which runs on the device on any batch.  ValueError
    otherwise (main turns it into a parser error)."""
    if augment is None:
        return
    if args.kitti_flow:
        raise ValueError("--augment / --aug-* do not apply with --kitti-flow: a spatial "
                         "augmentation would have to move the ground truth with the frame")
    if not args.kitti and not args.selfsup_weight > 0:
        raise ValueError("--augment / --aug-* apply only with --kitti: without it the driver "
                         "trains on synthetic pairs, which are not augmented")


def check_selfsup_args(args):
    """--selfsup-weight > 0 needs --warp-convention image (an augmentation can only carry an
    image displacement) and a transform to self-supervise with (--augment or an --aug-* flag);
    --selfsup-q is in (0, 2], --selfsup-eps > 0, --selfsup-start-epoch >= 0.  ValueError
    otherwise (main turns it into a parser error)."""
    if args.selfsup_weight < 0:
        raise ValueError("--selfsup-weight must be >= 0, got %r" % (args.selfsup_weight,))
    if not 0 < args.selfsup_q <= 2:
        raise ValueError("--selfsup-q must be in (0, 2], got %r" % (args.selfsup_q,))
    if not args.selfsup_eps > 0:
        raise ValueError("--selfsup-eps must be > 0, got %r" % (args.selfsup_eps,))
    if args.selfsup_start_epoch < 0:
        raise ValueError("--selfsup-start-epoch must be >= 0, got %d" % args.selfsup_start_epoch)
    if args.selfsup_weight > 0:
        if args.warp_convention != "image":
            raise ValueError("--selfsup-weight > 0 needs --warp-convention image: a "
                             "reference-convention flow is not an image displacement, an "
                             "augmentation cannot carry it")
        if augment_from_args(args) is None:
            raise ValueError("--selfsup-weight > 0 needs a transform to self-supervise with: "
                             "--augment or an --aug-* flag")


def check_occlusion_args(args):
    """--occlusion masks are defined on image displacements, so anything but "none" needs
    --warp-convention image; the alphas are >= 0.  ValueError otherwise (main turns it into a
    parser error)."""
    if args.occ_alpha1 < 0 or args.occ_alpha2 < 0:
        raise ValueError("--occ-alpha1 and --occ-alpha2 must be >= 0, got %r and %r"
                         % (args.occ_alpha1, args.occ_alpha2))
    if args.occlusion != "none" and args.warp_convention != "image":
        raise ValueError("--occlusion %s needs --warp-convention image: a reference-convention "
                         "flow is not a displacement, where the pixel went has no meaning"
                         % args.occlusion)


def header_record(args, augment=None, label_augment=None):
    """The step log's header record (no "step" key) for a run with any non-default loss,
    augmentation, clipping or warp-convention option; None for a default run, whose log holds
    step records only.  ``label_augment``: the AugmentOpts of the labelled frames
    (kitti_flow_augment_from_args), recorded as "kitti_flow_augment" when set."""
    census = (args.census_weight != 0.0 or args.census_radius != 3 or
              args.photometric_weight != 1.0)
    clip = args.clip_norm is not None or args.skip_nonfinite or args.log_grad_norm
    image = args.warp_convention == "image"
    occ = (args.occlusion != "none" or args.occ_alpha1 != 0.01 or args.occ_alpha2 != 0.5)
    order2 = getattr(args, "smoothness_order", 1) == 2
    ssim = getattr(args, "ssim_weight", 0.0)
    sup = getattr(args, "supervised_weight", 0.0)
    selfw = getattr(args, "selfsup_weight", 0.0)
    if not (args.smoothness_weight or args.edge_alpha or augment is not None or census or clip
            or image or occ or order2 or ssim or sup or selfw or label_augment is not None):
        return None
    head = {"header": True, "smoothness_weight": args.smoothness_weight,
            "edge_alpha": args.edge_alpha}
    if order2:                      # first-order logs stay what they were
        head["smoothness_order"] = 2
    if ssim:                        # logs without the SSIM term stay what they were
        head["ssim_weight"] = ssim
    if sup:                         # logs without the supervised term stay what they were
        head.update(supervised_weight=sup, supervised_q=args.supervised_q,
                    supervised_eps=args.supervised_eps, kitti_flow=args.kitti_flow,
                    kitti_flow_holdout=args.kitti_flow_holdout)
    if selfw:                       # logs without self-supervision stay what they were
        head["selfsup"] = {"weight": selfw, "q": args.selfsup_q, "eps": args.selfsup_eps,
                           "start_epoch": args.selfsup_start_epoch}
    if census:
        head.update(census_weight=args.census_weight, census_radius=args.census_radius,
                    photometric_weight=args.photometric_weight)
    if augment is not None:
        head["augment"] = augment.as_dict()
    if label_augment is not None:   # logs without labelled augmentation stay what they were
        head["kitti_flow_augment"] = label_augment.as_dict()
    if clip:
        head.update(clip_norm=args.clip_norm, skip_nonfinite=args.skip_nonfinite,
                    log_grad_norm=args.log_grad_norm)
    if image:
        head["warp_convention"] = args.warp_convention
    if occ:
        head.update(occlusion=args.occlusion, occ_alpha1=args.occ_alpha1,
                    occ_alpha2=args.occ_alpha2)
    if args.eval_kitti_flow is not None:
        head.update(eval_kitti_flow=args.eval_kitti_flow, eval_every=args.eval_every)
    return head


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    try:
        augment = augment_from_args(args)
        label_augment = kitti_flow_augment_from_args(args)
    except ValueError as e:
        ap.error(str(e))
    try:
        check_augment_args(args, augment)
        check_kitti_flow_augment_args(args, label_augment)
        check_eval_args(args)
        check_occlusion_args(args)
        check_supervised_args(args)
        check_selfsup_args(args)
    except ValueError as e:
        ap.error(str(e))

    try:
        loss_layer = LossLayer(args.smoothness_weight, args.edge_alpha,
                               census_weight=args.census_weight,
                               census_radius=args.census_radius,
                               photometric_weight=args.photometric_weight,
                               warp_convention=args.warp_convention,
                               occlusion=args.occlusion, occlusion_alpha1=args.occ_alpha1,
                               occlusion_alpha2=args.occ_alpha2,
                               smoothness_order=args.smoothness_order,
                               ssim_weight=args.ssim_weight,
                               supervised_weight=args.supervised_weight,
                               supervised_q=args.supervised_q,
                               supervised_eps=args.supervised_eps,
                               selfsup_weight=args.selfsup_weight, selfsup_q=args.selfsup_q,
                               selfsup_eps=args.selfsup_eps)
    except ValueError as e:
        ap.error(str(e))
    try:
        KerasAdam.check_global_clipnorm(args.clip_norm)
    except ValueError as e:
        ap.error("--clip-norm: " + str(e))
    clip = args.clip_norm is not None or args.skip_nonfinite or args.log_grad_norm

    rank, world, local = init_from_env()
    torch.cuda.set_device(local)
    net = build_flow_net(args.height, args.width, args.pretrained, seed=args.seed,
                         warp_convention=args.warp_convention)
    if rank == 0:
        net.summary()
    opt = KerasAdam(net.store, learning_rate=args.lr, global_clipnorm=args.clip_norm,
                    skip_nonfinite=args.skip_nonfinite, track_grad_norm=args.log_grad_norm)
    selfsup = args.selfsup_weight > 0
    # with self-supervision the augmentation flags set its transform (on the device, seeded per
    # rank like the reader); the reader then hands out the frames as they are
    trainer = Trainer(net, opt, loss_layer, selfsup=augment if selfsup else None,
                      selfsup_seed=args.seed + rank)
    log = open(args.log, "a") if (args.log and rank == 0) else None
    head = header_record(args, augment, label_augment)
    if log and head is not None:
        log.write(json.dumps(head) + "\n")
    reader = None
    if args.kitti:
        from .data_reader import AsyncReader, ReaderOpts
        reader = AsyncReader(ReaderOpts(args.kitti, args.batch, args.height, args.width,
                                        args.nworkers, seed=args.seed + rank,
                                        augment=None if selfsup else augment))
    labelled = None
    eval_frames = None
    if args.kitti_flow:
        from .evaluate import KittiFlowReader, evaluate, list_kitti_flow, split_kitti_flow
        frames = list_kitti_flow(args.kitti_flow)
        if args.kitti_flow_holdout:
            frames, held = split_kitti_flow(frames, args.kitti_flow_holdout)
            if rank == 0:
                eval_frames = held
        labelled = KittiFlowReader(frames, args.batch, args.height, args.width,
                                   nworkers=args.nworkers, seed=args.seed + rank,
                                   label_augment=label_augment)
    nbatches = (reader.nbatches if reader is not None else
                labelled.nbatches if labelled is not None else args.steps)
    if args.eval_kitti_flow is not None and rank == 0:
        from .evaluate import evaluate, list_kitti_flow
        eval_frames = list_kitti_flow(args.eval_kitti_flow)      # a bad root fails before training
    step = 0
    for epoch in range(args.epochs):
        if epoch == args.lr_drop_epoch:
            opt.learning_rate = args.lr * 0.1
        if selfsup:
            trainer.selfsup_enabled = epoch >= args.selfsup_start_epoch
        t0 = time.time()
        epoch_batches = iter(labelled) if labelled is not None else None
        for b in range(nbatches):
            gt = None
            if epoch_batches is not None:
                batch, gt_raw, descs = next(epoch_batches)
                if args.supervised_weight > 0:
                    gt = (gt_raw, descs)
            elif reader is not None:
                batch = reader.get_batch()
            else:
                batch = torch.from_numpy(synthetic_batch(args.batch, args.height, args.width,
                                                         seed=1234 + step, rank=rank)).cuda()
            loss, flows = trainer.train_step(batch, step, gt=gt)
            lv = float(loss)
            if rank == 0:
                sys.stdout.write("\rbatch %d/%d, loss: %.2e    " % (b + 1, nbatches, lv))
                sys.stdout.flush()
                if log:
                    rec = {"step": step, "loss": lv, "t": time.time() - t0}
                    if clip:
                        # read where the loss was just read (the step is complete): the state
                        # block of this step, no further sync point
                        rec["grad_norm"] = float(opt.last_grad_norm)
                        rec["skipped"] = opt.skipped_updates
                    log.write(json.dumps(rec) + "\n")
                if args.display_dir and (b + 1) % 10 == 0:
                    from .drawing import display_training
                    shown = batch
                    if selfsup and trainer.selfsup_enabled:      # the batch the flows belong to
                        shown = trainer.last_selfsup["batch"]
                    display_training(shown, flows, args.display_dir, step)
            step += 1
        if rank == 0:
            print("\nEpoch computed in %.3fs" % (time.time() - t0))
            if args.save_dir:
                net.save_weights(os.path.join(args.save_dir, "flow_net_%d" % epoch, "weights"))
            if eval_frames is not None and ((epoch + 1) % args.eval_every == 0 or
                                            epoch == args.epochs - 1):
                res = evaluate(net, eval_frames, nworkers=args.nworkers)
                res.pop("per_image")
                line = json.dumps({"eval": res, "epoch": epoch})
                print(line, flush=True)
                if log:
                    log.write(line + "\n")
    if log:
        log.close()
    if reader is not None:
        reader.close()


if __name__ == "__main__":
    main()
