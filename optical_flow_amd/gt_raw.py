"""The raw ground-truth batch of KITTI flow maps (include/oflow.h, of_flow_eval): what the
evaluation (evaluate.py) and the supervised loss term (ops.supervised_flow_loss) both hand to
their kernels.  Here so that neither imports the other."""
from __future__ import annotations

import numpy as np
import torch

# of_image_desc (include/oflow.h)
DESC_DTYPE = np.dtype([("offset", np.int64), ("h", np.int32), ("w", np.int32)])
assert DESC_DTYPE.itemsize == 16


def pack_gt_raw(maps):
    """[(h_i, w_i, 3) uint16, ...] -> (raw uint8 buffer, descriptors): of_image_desc[n] padded to
    256 bytes, then the maps, each at a 256-byte aligned offset (the raw image batch's layout)."""
    n = len(maps)
    total = -(-16 * n // 256) * 256
    desc = np.zeros(n, DESC_DTYPE)
    for i, m in enumerate(maps):
        if m.dtype != np.uint16 or m.ndim != 3 or m.shape[2] != 3:
            raise ValueError("ground-truth map %d must be (h, w, 3) uint16, got %s %r" %
                             (i, m.dtype, m.shape))
        desc[i] = (total, m.shape[0], m.shape[1])
        total += -(-m.nbytes // 256) * 256
    raw = np.zeros(max(total, 256), np.uint8)
    raw[:16 * n] = desc.view(np.uint8)
    for d, m in zip(desc, maps):
        raw[d["offset"]:d["offset"] + m.nbytes] = np.ascontiguousarray(m).reshape(-1).view(np.uint8)
    return raw, desc


def _upload(host: np.ndarray) -> torch.Tensor:
    """A host byte buffer to the GPU without a host wait: staged in pinned memory (torch's host
    allocator keeps a block until the copy that reads it has completed), copied non_blocking on
    the current stream."""
    staged = torch.empty(host.size, dtype=torch.uint8, pin_memory=True)
    staged.numpy()[:] = host.reshape(-1)
    return staged.cuda(non_blocking=True)


def device_gt(gt_raw, descs, n):
    """The ground truth of ``n`` images as (CUDA uint8 buffer, host descriptors) from a list of n
    (h, w, 3) uint16 maps, or pack_gt_raw's buffer (numpy or already on the GPU) with its
    descriptors.  Host ground truth is uploaded by an asynchronous copy from pinned staging."""
    if isinstance(gt_raw, (list, tuple)):
        gt_raw, descs = pack_gt_raw(gt_raw)
    if isinstance(gt_raw, np.ndarray):
        if descs is None:
            descs = gt_raw[:16 * n].view(DESC_DTYPE).copy()
        gt_raw = _upload(gt_raw)
    if descs is None:
        raise ValueError("a device ground-truth buffer needs its host descriptors")
    descs = np.ascontiguousarray(descs, dtype=DESC_DTYPE)
    if not (torch.is_tensor(gt_raw) and gt_raw.is_cuda and gt_raw.dtype == torch.uint8):
        raise ValueError("the ground-truth buffer must be a CUDA uint8 tensor")
    if len(descs) != n:
        raise ValueError("%d descriptors for %d flows" % (len(descs), n))
    return gt_raw, descs
