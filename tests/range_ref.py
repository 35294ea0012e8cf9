"""The range-map occlusion mask restated from its definition (DESIGN.md "Range-map occlusion";
include/oflow.h of_occ_range_multi), in whatever dtype the inputs have (float64 in the tests),
image convention only.  For a doubled batch [forward ; swapped] of n flows, image b with partner
b' = (b + n/2) % n and g the partner's flow:

    for every pixel q = (i, j):  x = j + g0[q], y = i + g1[q]     (formed in float32, as
                                                                   occlusion_ref.sample_points)
        x0 = floor(x), y0 = floor(y), fx = x - x0, fy = y - y0
        the taps (y0 + dy, x0 + dx), dy, dx in {0, 1}, weigh (1 - fy | fy) * (1 - fx | fx);
        a tap outside [0, h-1] x [0, w-1] is dropped, a non-finite point contributes nothing
    R_b[p]    = sum of the tap weights that land on p
    mask_b[p] = border(f_b)[p] * min(1, R_b[p])

Not a test module: the range tests import it.  It also holds their shared inputs."""
import torch

import occlusion_ref as O
from occlusion_ref import _rng_tensor, border, census, near, photometric  # noqa: F401


def _taps(flow, keep=None):
    """Per tap (dy, dx): (destination index into h*w, weight, landed) of every source pixel of
    the PARTNER of each image, each (n, h*w).  ``keep`` (n,h,w) bool, indexed like ``flow``:
    the source pixels that take part (None: all)."""
    n, h, w, _ = flow.shape
    assert n % 2 == 0
    partner = torch.roll(flow, -(n // 2), 0)            # image b receives from (b + n/2) % n
    x, y = O.sample_points(partner)
    ok = torch.isfinite(x) & torch.isfinite(y)
    if keep is not None:
        ok = ok & torch.roll(keep, -(n // 2), 0)
    x0, y0 = torch.floor(x), torch.floor(y)
    fx, fy = x - x0, y - y0
    for dy in (0, 1):
        for dx in (0, 1):
            ty, tx = y0 + dy, x0 + dx
            wt = (fy if dy else 1 - fy) * (fx if dx else 1 - fx)
            lands = ok & (ty >= 0) & (ty <= h - 1) & (tx >= 0) & (tx <= w - 1)
            idx = torch.where(lands, ty * w + tx, torch.zeros_like(ty)).long()
            wt = torch.where(lands, wt, torch.zeros_like(wt))
            yield idx.reshape(n, -1), wt.reshape(n, -1), lands.reshape(n, -1)


def range_map(flow, keep=None):
    """R (n,h,w) of a doubled batch."""
    n, h, w, _ = flow.shape
    R = flow.new_zeros(n, h * w)
    for idx, wt, _ in _taps(flow, keep):
        R.scatter_add_(1, idx, wt)
    return R.reshape(n, h, w)


def tap_counts(flow):
    """(n,h,w) int64: how many taps of non-zero weight land on each pixel."""
    n, h, w, _ = flow.shape
    cnt = torch.zeros(n, h * w, dtype=torch.int64)
    for idx, wt, lands in _taps(flow):
        cnt.scatter_add_(1, idx, (lands & (wt > 0)).long())
    return cnt.reshape(n, h, w)


def mask(flow, keep=None):
    return border(flow)[0] * range_map(flow, keep).clamp(max=1.0)


def masks(flows):
    """ops.occlusion_masks(flows, "range"): per pyramid level a (n,h,w) weight in [0, 1]."""
    return [mask(f) for f in flows]


# ----------------------------------------------------- the inputs of the range tests ----
ABI_LEVELS = O.ABI_LEVELS                   # [(1, 1), (5, 3), (13, 21), (40, 57)]
ABI_N = 4                                   # B = 2: two pairs with different flows
ABI_SCALE = 0.3
LAYER_SCALE = 0.3


def abi_flows(scale=ABI_SCALE):
    """float32 flows of the ABI test, one per ABI_LEVELS entry."""
    return [_rng_tensor((ABI_N, h, w, 2), 300 + h, scale) for h, w in ABI_LEVELS]


def layer_case():
    """(batch (4,48,80,6), four float32 flow levels) of the LossLayer parity test: the doubled
    batch of occlusion_ref.layer_case("fb"), flows with no pixel within 1e-3 of a border
    decision (the only discontinuity of the range mask)."""
    batch, _ = O.layer_case("fb")
    n, H, W = O.LAYER_SIZE["fb"]
    flows = [_rng_tensor((n, H >> (s + 1), W >> (s + 1), 2), O.LAYER_SEED + s, LAYER_SCALE)
             for s in range(4)]
    return batch, [O._condition(f, "border", 0.0) for f in flows]


def _grid(h, w):
    ii, jj = torch.meshgrid(torch.arange(h, dtype=torch.float32),
                            torch.arange(w, dtype=torch.float32), indexing="ij")
    return torch.stack([jj, ii], -1)                    # channel 0 along x, channel 1 along y


def known_flows(h, w, B=2):
    """name -> float32 (2B,h,w,2) flows whose range maps are known exactly (every tap weight is
    0, 0.25, 0.5 or 1): zero; forward (+2, 0) with backward (-2, 0); forward 0 with backward
    -q/2 (the points q/2); forward 0 with backward +q (the points 2q)."""
    z = torch.zeros(2 * B, h, w, 2)
    shift = z.clone()
    shift[:B, ..., 0], shift[B:, ..., 0] = 2.0, -2.0
    contract, expand = z.clone(), z.clone()
    contract[B:] = -0.5 * _grid(h, w)
    expand[B:] = _grid(h, w)
    return {"zero": z, "shift": shift, "contract": contract, "expand": expand}


def edge_flows(h=13, w=21, seed=77):
    """(flow with NaN, +-inf and +-1e9 entries at a few source pixels, the same flow with those
    entries 0, keep (n,h,w): False at those pixels)."""
    clean = _rng_tensor((ABI_N, h, w, 2), seed, ABI_SCALE)
    bad = clean.clone()
    keep = torch.ones(ABI_N, h, w, dtype=torch.bool)
    inf = float("inf")
    for k, (b, i, j, c, v) in enumerate([(0, 0, 0, 0, float("nan")), (1, 3, 4, 1, inf),
                                         (2, 6, 20, 0, -inf), (3, 12, 0, 1, 1e9),
                                         (2, 5, 5, 0, -1e9), (3, 12, 20, 1, float("nan")),
                                         (0, 7, 9, 0, 1e9), (1, 2, 2, 1, -1e9)]):
        bad[b, i, j, c] = v
        clean[b, i, j, c] = 0.0
        keep[b, i, j] = False
    return bad, clean, keep
