"""Mirror of the reference ``loss.py`` (LossLayer, loss.py:5-32)."""
from __future__ import annotations

from . import ops


class LossLayer:
    """Multi-scale photometric L1: for scale s, resize the (B,H,W,6) pairs to H/2^(s+1),
    warp image2 by flows[s] with ``warp_features``' convention, mean |image1 - warped| over
    B*h*w*3, averaged over scales (P10).  HIP: one pyramid kernel per level, one fused
    warp+|diff|+reduce kernel per scale, and a d(flow) kernel per scale for the backward.

    ``LossLayer()`` is the reference's layer.  ``smoothness_weight`` > 0 (build-added) adds
    that weight times the edge-aware first-order smoothness of every scale's flow: the mean
    Charbonnier penalty sqrt(d^2 + smoothness_eps) of the vertical plus that of the horizontal
    first differences, each weighted by exp(-edge_alpha * mean |d image1|) across the same
    pixel pair, averaged over scales (ops.flow_loss; DESIGN.md has the definition).
    ``smoothness_order`` = 2 (build-added) penalises the second differences f[p-1] - 2 f[p] +
    f[p+1] instead, weighted across each triple's two outer pixels: a flow that is affine in
    image coordinates (a plane seen in perspective) then costs nothing (DESIGN.md
    "Second-order smoothness").  It plays no part while ``smoothness_weight`` is 0.

    ``census_weight`` > 0 (build-added) adds that weight times the soft ternary census term,
    an illumination-robust data term that compares the local intensity order of image 1 and
    of the warped image 2 in a (2 census_radius + 1)^2 window, averaged over pixels and scales
    (ops.census_loss; DESIGN.md "Census term").  ``photometric_weight`` scales the photometric
    term; 0 drops it (its kernels are not launched), which needs another data term.

    ``ssim_weight`` > 0 (build-added) adds that weight times the structural-similarity term:
    the mean over scales, over the 3 x 3 windows that lie inside the image and over channels
    of (1 - SSIM)/2 between image 1 and the warped image 2, on intensities (the channel means
    added back), with C1 = 0.01^2, C2 = 0.03^2 and no clamp (ops.ssim_loss; DESIGN.md "SSIM
    term").  The usual mix is ``photometric_weight=0.15, ssim_weight=0.85``.  The loss needs
    at least one of the three data weights to be non-zero.

    ``warp_convention`` (build-added): "reference" (default) warps image 2 on the reference's
    transposed grid (P1); "image" takes the flows as image-coordinate displacements (channel 0
    along x, channel 1 along y) in the photometric and the census term, so the true motion
    brings the loss to zero.  It must be the net's (Trainer raises ValueError otherwise).

    ``occlusion`` (build-added, image convention only): "none" (default) scores every pixel;
    "border" gives weight 0 in the data terms (SSIM: to the window centred there) to the
    pixels whose sample point leaves the frame (where the warp extrapolates); "fb" also to those that fail the forward-backward
    consistency check |f + g~|^2 <= occlusion_alpha1 (|f|^2 + |g~|^2) + occlusion_alpha2
    (alpha2 in squared full-resolution pixels), and must be called with the doubled batch
    [pairs ; the same pairs with the two images exchanged] (Trainer.train_step forms it).  The
    masks are computed from the flows as constants (ops.occlusion_masks; DESIGN.md "Occlusion
    masks"); the means stay over all pixels and the smoothness term is not masked.
    "range" (the doubled batch again, wherever "fb" needs it) weighs the data terms by the soft
    range-map mask of Wang et al. (CVPR 2018): every pixel of image 2 is moved by the backward
    flow and splatted bilinearly into image 1, and a pixel's weight is min(1, what landed on it)
    times the border mask, a float in [0, 1] with no thresholds (``occlusion_alpha1`` and
    ``occlusion_alpha2`` play no part; ops.range_map, DESIGN.md "Range-map occlusion").

    ``supervised_weight`` > 0 (build-added, image convention only) adds that weight times the
    supervised term against KITTI flow ground truth, passed to the call as ``gt`` (a list of
    (h, w, 3) uint16 maps, pack_gt_raw's buffer, or (buffer, descriptors)): per scale the
    flow is upsampled to each map's native size as the evaluation samples it, and the
    Charbonnier end-point error (|u - gt|^2 + supervised_eps^2)^(supervised_q / 2), in native
    pixels, is averaged over an image's valid pixels, then over the images that have one, then
    over the scales with ``supervised_level_weights`` (default 1 / scales each)
    (ops.supervised_flow_loss; DESIGN.md "Supervised term").  With it the three unsupervised
    data weights may all be 0 (pure fine-tuning).  With ``occlusion="fb"`` or ``"range"`` it
    scores the forward pairs only (the first half of the doubled batch); the occlusion masks do
    not weigh it.

    ``selfsup_weight`` > 0 (build-added, image convention only) adds that weight times the
    self-supervision term: the finest flow against a target that ops.transform_flow carried over
    from a teacher pass on the un-augmented batch, passed to the call as ``selfsup`` = (target,
    weight); the penalty weight * (|flow - target|^2 + selfsup_eps^2)^(selfsup_q / 2) is averaged
    over all cells of the target's images (ops.selfsup_flow_loss; DESIGN.md "Self-supervision";
    Trainer(selfsup=...) runs the teacher pass).  It is no data term: the loss still needs one."""

    def __init__(self, smoothness_weight=0.0, edge_alpha=0.0, smoothness_eps=1e-4,
                 census_weight=0.0, census_radius=3, photometric_weight=1.0,
                 warp_convention="reference", occlusion="none", occlusion_alpha1=0.01,
                 occlusion_alpha2=0.5, ssim_weight=0.0, supervised_weight=0.0,
                 supervised_q=1.0, supervised_eps=0.01, supervised_level_weights=None,
                 selfsup_weight=0.0, selfsup_q=0.4, selfsup_eps=0.01, smoothness_order=1):
        ops.warp_convention(warp_convention)
        self.warp_convention = warp_convention
        if occlusion not in ("none", "border", "fb", "range"):
            raise ValueError("occlusion must be 'none', 'border', 'fb' or 'range', got %r"
                             % (occlusion,))
        if not occlusion_alpha1 >= 0:
            raise ValueError("occlusion_alpha1 must be >= 0, got %r" % (occlusion_alpha1,))
        if not occlusion_alpha2 >= 0:
            raise ValueError("occlusion_alpha2 must be >= 0, got %r" % (occlusion_alpha2,))
        if occlusion != "none" and warp_convention != "image":
            raise ValueError("occlusion=%r needs warp_convention='image': a %r-convention flow "
                             "is not a displacement" % (occlusion, warp_convention))
        self.occlusion = occlusion
        self.occlusion_alpha1 = float(occlusion_alpha1)
        self.occlusion_alpha2 = float(occlusion_alpha2)
        if not smoothness_weight >= 0:
            raise ValueError("smoothness_weight must be >= 0, got %r" % (smoothness_weight,))
        if not edge_alpha >= 0:
            raise ValueError("edge_alpha must be >= 0, got %r" % (edge_alpha,))
        if not smoothness_eps > 0:
            raise ValueError("smoothness_eps must be > 0, got %r" % (smoothness_eps,))
        if not census_weight >= 0:
            raise ValueError("census_weight must be >= 0, got %r" % (census_weight,))
        if not photometric_weight >= 0:
            raise ValueError("photometric_weight must be >= 0, got %r" % (photometric_weight,))
        if census_radius not in (1, 2, 3):
            raise ValueError("census_radius must be 1, 2 or 3, got %r" % (census_radius,))
        if not ssim_weight >= 0:
            raise ValueError("ssim_weight must be >= 0, got %r" % (ssim_weight,))
        if not supervised_weight >= 0:
            raise ValueError("supervised_weight must be >= 0, got %r" % (supervised_weight,))
        if not 0 < supervised_q <= 2:
            raise ValueError("supervised_q must be in (0, 2], got %r" % (supervised_q,))
        if not supervised_eps > 0:
            raise ValueError("supervised_eps must be > 0, got %r" % (supervised_eps,))
        if supervised_level_weights is not None:
            supervised_level_weights = tuple(float(v) for v in supervised_level_weights)
            if not supervised_level_weights or not all(v >= 0 for v in supervised_level_weights):
                raise ValueError("supervised_level_weights must be a non-empty sequence of "
                                 "values >= 0, got %r" % (supervised_level_weights,))
        if supervised_weight > 0 and warp_convention != "image":
            raise ValueError("supervised_weight > 0 needs warp_convention='image': a "
                             "%r-convention flow is not a displacement, its error against "
                             "ground truth means nothing" % (warp_convention,))
        if not selfsup_weight >= 0:
            raise ValueError("selfsup_weight must be >= 0, got %r" % (selfsup_weight,))
        if not 0 < selfsup_q <= 2:
            raise ValueError("selfsup_q must be in (0, 2], got %r" % (selfsup_q,))
        if not selfsup_eps > 0:
            raise ValueError("selfsup_eps must be > 0, got %r" % (selfsup_eps,))
        if selfsup_weight > 0 and warp_convention != "image":
            raise ValueError("selfsup_weight > 0 needs warp_convention='image': a %r-convention "
                             "flow is not a displacement, an augmentation cannot carry it"
                             % (warp_convention,))
        self.selfsup_weight = float(selfsup_weight)
        self.selfsup_q = float(selfsup_q)
        self.selfsup_eps = float(selfsup_eps)
        self.supervised_weight = float(supervised_weight)
        self.supervised_q = float(supervised_q)
        self.supervised_eps = float(supervised_eps)
        self.supervised_level_weights = supervised_level_weights
        if census_weight == 0 and photometric_weight == 0 and ssim_weight == 0 and \
                supervised_weight == 0:
            raise ValueError("census_weight, photometric_weight and ssim_weight are all 0: the "
                             "loss needs a data term")
        if smoothness_order not in (1, 2) or isinstance(smoothness_order, bool):
            raise ValueError("smoothness_order must be 1 or 2, got %r" % (smoothness_order,))
        self.smoothness_order = int(smoothness_order)
        self.smoothness_weight = float(smoothness_weight)
        self.edge_alpha = float(edge_alpha)
        self.smoothness_eps = float(smoothness_eps)
        self.census_weight = float(census_weight)
        self.census_radius = int(census_radius)
        self.photometric_weight = float(photometric_weight)
        self.ssim_weight = float(ssim_weight)

    def __call__(self, batch_imgs, flows, gt=None, selfsup=None):
        if self.selfsup_weight > 0 and selfsup is None:
            raise ValueError("selfsup_weight > 0: the call needs the (target, weight) pair "
                             "(selfsup)")
        if self.selfsup_weight == 0 and selfsup is not None:
            raise ValueError("self-supervision target given, but selfsup_weight is 0")
        if self.supervised_weight > 0 and gt is None:
            raise ValueError("supervised_weight > 0: the call needs the ground truth (gt)")
        if self.supervised_weight == 0 and gt is not None:
            raise ValueError("ground truth given, but supervised_weight is 0")
        num_scales = len(flows)
        H, W = batch_imgs.shape[1], batch_imgs.shape[2]
        for scale_idx in range(num_scales):
            scaled_height = int(H / (2.0 ** (scale_idx + 1)))
            scaled_width = int(W / (2.0 ** (scale_idx + 1)))
            assert flows[scale_idx].shape[1] == scaled_height
            assert flows[scale_idx].shape[2] == scaled_width
        assert batch_imgs.shape[3] == 6
        # the first order is the ops entries' default: such a layer calls them as it always did
        order = {"smoothness_order": 2} if self.smoothness_order == 2 else {}
        if self.ssim_weight != 0.0:     # without it the ops entries are called as before
            order["ssim_weight"] = self.ssim_weight
        if self.selfsup_weight != 0.0:
            order.update(selfsup_weight=self.selfsup_weight, selfsup_q=self.selfsup_q,
                         selfsup_eps=self.selfsup_eps, selfsup=selfsup)
        if self.supervised_weight != 0.0:
            if self.supervised_level_weights is not None and \
                    len(self.supervised_level_weights) != num_scales:
                raise ValueError("supervised_level_weights has %d values for %d flows"
                                 % (len(self.supervised_level_weights), num_scales))
            order.update(supervised_weight=self.supervised_weight,
                         supervised_q=self.supervised_q, supervised_eps=self.supervised_eps,
                         supervised_level_weights=self.supervised_level_weights,
                         gt=self._forward_gt(gt, batch_imgs.shape[0]))
            if self.occlusion == "none":
                return ops.census_flow_loss(batch_imgs, list(flows), self.census_weight,
                                            self.census_radius, self.photometric_weight,
                                            self.smoothness_weight, self.edge_alpha,
                                            self.smoothness_eps, self.warp_convention, **order)
        if self.occlusion != "none":
            if ops.needs_swapped_pairs(self.occlusion) and batch_imgs.shape[0] % 2:
                raise ValueError("occlusion=%r scores the doubled batch [pairs ; swapped "
                                 "pairs]: an even number of images, got %d"
                                 % (self.occlusion, batch_imgs.shape[0]))
            masks = ops.occlusion_masks([f.detach() for f in flows], self.occlusion,
                                        self.occlusion_alpha1, self.occlusion_alpha2,
                                        self.warp_convention)
            return ops.census_flow_loss(batch_imgs, list(flows), self.census_weight,
                                        self.census_radius, self.photometric_weight,
                                        self.smoothness_weight, self.edge_alpha,
                                        self.smoothness_eps, self.warp_convention, weights=masks,
                                        **order)
        if self.census_weight == 0.0 and self.photometric_weight == 1.0 and \
                self.ssim_weight == 0.0 and self.selfsup_weight == 0.0:
            if self.smoothness_weight == 0.0:
                return ops.photometric_loss(batch_imgs, list(flows), self.warp_convention)
            return ops.flow_loss(batch_imgs, list(flows), self.smoothness_weight,
                                 self.edge_alpha, self.smoothness_eps, self.warp_convention,
                                 **order)
        return ops.census_flow_loss(batch_imgs, list(flows), self.census_weight,
                                    self.census_radius, self.photometric_weight,
                                    self.smoothness_weight, self.edge_alpha,
                                    self.smoothness_eps, self.warp_convention, **order)

    def _forward_gt(self, gt, nb):
        """The ground truth as ops takes it; with occlusion="fb" or "range" it belongs to the
        forward pairs, the first half of the doubled batch."""
        n = nb // 2 if ops.needs_swapped_pairs(self.occlusion) else nb
        return ops._gt_handle(gt, n)
