"""Global-norm gradient clipping and the non-finite update guard on the GPU: the deterministic
sum of squares of the gradient arena (of_grad_sumsq) against numpy, the clipped Keras Adam
(of_adam_keras_dev_clip, KerasAdam(global_clipnorm=..., skip_nonfinite=..., track_grad_norm=...))
against the oracle's Adam fed float64-clipped gradients, the bitwise no-op and skip properties,
the whole train step against the oracle, and the captured (HIP graph) and data-parallel steps.
Non-finite values are only ever written into the gradient arena after the backward; none goes
through the network's kernels."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from helpers import REL_TOL, dev, rel_inf, rel_l2, rng_tensor
from oracle import ref_flow as R

pytestmark = pytest.mark.gpu

N_FULL = 4937219                      # the flow net's 4.94 M parameters, not a multiple of 4


def _lib():
    from optical_flow_amd import _lib
    return _lib.lib()


def _vp(t):
    return C.c_void_p(t.data_ptr())


# -------------------------------------------------------------- the sum of squares ------
def _layout(n):
    """(P, [(lo, hi)] per workgroup): the ranges include/oflow.h documents, from
    of_grad_sumsq_partials."""
    P = _lib().of_grad_sumsq_partials(n)
    nq = n // 4
    chunk = -(-nq // P)
    r = [(min(4 * b * chunk, 4 * nq), min(4 * (b + 1) * chunk, 4 * nq)) for b in range(P)]
    r[-1] = (r[-1][0], n)
    return P, r


class _Bench:
    """One set of device arenas of N_FULL + 8 floats, reused by every size."""

    def __init__(self):
        from optical_flow_amd import ops
        self.ops = ops
        self.cap = N_FULL + 8
        self.host = np.random.default_rng(11).standard_normal(self.cap).astype(np.float32)
        self.sq = self.host.astype(np.float64) ** 2            # exact
        self.g = torch.from_numpy(self.host).cuda()
        self.p, self.m, self.v = (torch.zeros(self.cap, device="cuda") for _ in range(3))
        self.sched = torch.zeros(2, device="cuda")             # lr 0: p stays
        self.it = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.state = torch.zeros(_lib().of_adam_clip_state_bytes() // 8, dtype=torch.float64,
                                 device="cuda")

    def run(self, g, n, gs=1.0, clip=0.0, skip=0):
        """of_grad_sumsq + of_adam_keras_dev_clip over g[:n]; returns (partials with their
        guard words, double norm, float norm, mult, skip)."""
        from optical_flow_amd._lib import call
        P = _lib().of_grad_sumsq_partials(n)
        buf = torch.full((P + 2,), 7.0, dtype=torch.float64, device="cuda")
        part = buf[1:P + 1]
        st = self.ops._stream()
        call("of_grad_sumsq", _vp(g), n, _vp(part), st)
        call("of_adam_keras_dev_clip", _vp(self.p), _vp(g), _vp(self.m), _vp(self.v), n,
             _vp(self.sched), _vp(self.it), 0.9, 0.999, 1e-7, gs, _vp(part), P, clip, skip,
             _vp(self.state), st)
        torch.cuda.synchronize()
        s = self.state.cpu()
        f = s.view(torch.float32)
        return buf.cpu().numpy(), s[0].item(), f[2].item(), f[3].item(), s.view(torch.int32)[4].item()


@pytest.fixture(scope="module")
def bench():
    return _Bench()


def _check_size(bench, n):
    buf, norm, norm_f, mult, skip = bench.run(bench.g, n)
    P, ranges = _layout(n)
    assert buf[0] == 7.0 and buf[-1] == 7.0 and len(buf) == P + 2          # guard words
    ref = np.sqrt(np.sum(bench.sq[:n], dtype=np.longdouble))
    bound = (n - 1) * 2.0 ** -53 + 2.0 ** -52
    err = float(abs(np.longdouble(norm) - ref) / ref)
    print("n %d P %d norm %.17g rel err %.3e bound %.3e" % (n, P, norm, err, bound))
    assert err <= bound, (n, err, bound)
    assert norm_f == float(np.float32(norm))                  # the correctly rounded double
    assert mult == 1.0 and skip == 0
    # every workgroup's partial is the sum over its documented range; empty ranges store 0
    for b, (lo, hi) in enumerate(ranges):
        want = float(np.sum(bench.sq[lo:hi], dtype=np.longdouble))
        if hi <= lo:
            assert buf[1 + b] == 0.0, (n, b)
        else:
            assert abs(buf[1 + b] - want) <= want * (hi - lo) * 2.0 ** -53, (n, b, lo, hi)
    return P, ranges


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, N_FULL])
def test_sumsq_sizes(bench, n):
    """n = 1 ... 5: all workgroups but the first (its one quad) and the last (the scalar tail)
    own an empty range."""
    P, ranges = _check_size(bench, n)
    if n <= 5:
        assert 1 <= sum(1 for lo, hi in ranges if hi > lo) <= 2 and P >= 64


def test_sumsq_range_edges(bench):
    """Sizes at which a workgroup's range ends, from of_grad_sumsq_partials: for the full
    arena's layout, the array ending at the last index of the first and of the last
    workgroup's range and one element to either side; sizes whose quads divide evenly over
    the workgroups, one quad or one element more or less; and the sizes around which P starts
    to grow and stops growing."""
    lib = _lib()
    P, ranges = _layout(N_FULL)
    sizes = set()
    for lo, hi in (ranges[0], ranges[-1]):
        sizes.update((hi - 1, hi, hi + 1))                 # hi - 1 is the range's last index
        sizes.update((lo - 1, lo, lo + 1) if lo > 1 else ())
    for base in (1 << 12, N_FULL - 4000):
        Pb = lib.of_grad_sumsq_partials(base)
        even = base // (4 * Pb) * (4 * Pb)
        assert lib.of_grad_sumsq_partials(even) == Pb
        sizes.update((even - 4, even - 1, even, even + 1, even + 4))
    grow = [n for n in range(1 << 14, N_FULL, 1 << 14)
            if lib.of_grad_sumsq_partials(n) != lib.of_grad_sumsq_partials(n + 1)]
    assert grow, "P never changes below the full arena"
    sizes.update((grow[0], grow[0] + 1, grow[-1], grow[-1] + 1))
    sizes = sorted(s for s in sizes if 0 < s <= bench.cap)
    assert len(sizes) >= 20
    for n in sizes:
        _check_size(bench, n)


@pytest.mark.parametrize("n", [5, 100003, N_FULL])
def test_sumsq_extremes(bench, n):
    """|g| = 1e25 does not overflow, |g| = 1e-30 does not vanish (the squares are formed in
    double), zeros give exactly 0, one NaN / +inf / -inf anywhere gives NaN / inf / inf."""
    g = torch.empty(n, device="cuda")
    for val in (1e25, 1e-30):
        g.fill_(val)
        _, norm, norm_f, _, _ = bench.run(g, n)
        ref = np.longdouble(np.float32(val)) * np.sqrt(np.longdouble(n))
        assert math.isfinite(norm) and norm > 0.0
        assert float(abs(np.longdouble(norm) - ref) / ref) <= (n - 1) * 2.0 ** -53 + 2.0 ** -52
        assert norm_f == float(np.float32(norm)) and norm_f > 0.0 and math.isfinite(norm_f)
    g.zero_()
    buf, norm, norm_f, mult, _ = bench.run(g, n, clip=1.0)
    assert norm == 0.0 and norm_f == 0.0 and mult == 1.0 and not buf[1:-1].any()
    for pos in sorted({0, n // 2, n - 1}):                 # n - 1: the scalar tail
        for bad, want in ((float("nan"), "nan"), (float("inf"), "inf"), (float("-inf"), "inf")):
            g.copy_(bench.g[:n])
            g[pos] = bad
            for skip in (0, 1):
                _, norm, norm_f, mult, sk = bench.run(g, n, skip=skip)
                if want == "nan":
                    assert math.isnan(norm) and math.isnan(norm_f), (pos, bad)
                else:
                    assert norm == math.inf and norm_f == math.inf, (pos, bad)
                assert sk == skip and mult == 1.0


def test_sumsq_bitwise_repeatable(bench):
    a = bench.run(bench.g, N_FULL)
    b = bench.run(bench.g, N_FULL)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
    assert a[0][0] == 7.0 and a[0][-1] == 7.0


def test_clip_multiplier(bench):
    """The schedule kernel's multiplier: grad_scale bitwise at or under the threshold,
    grad_scale * clip / norm above it, NaN for a non-finite norm with the guard off."""
    n = 100003
    _, norm, _, _, _ = bench.run(bench.g, n)
    for gs in (1.0, 0.125, 1.0 / 3.0):
        gs32 = float(np.float32(gs))
        for factor in (4.0, 1.0000001, 0.5, 1e-3):
            clip = float(np.float32(norm * gs32 * factor))
            _, nm, _, mult, _ = bench.run(bench.g, n, gs=gs, clip=clip)
            assert abs(nm - gs32 * norm) <= 2.0 ** -52 * nm
            if nm <= clip:
                assert mult == gs32
            else:
                assert mult == float(np.float32(gs32 * clip / nm))
    g = bench.g[:n].clone()
    g[7] = float("inf")
    assert math.isnan(bench.run(g, n, clip=1.0, skip=0)[3])
    _, _, _, mult, sk = bench.run(g, n, clip=1.0, skip=1)
    assert sk == 1 and not math.isnan(mult)


# ------------------------------------------------------------- clipped Keras Adam -------
def _head_store():
    from optical_flow_amd.model import ParamStore
    from optical_flow_amd.params import head_spec, init_params
    spec = head_spec(3)
    vals = init_params(spec, 3)
    return ParamStore(spec, vals, device="cuda"), vals


def _head_grads(vals, it, mul=1.0):
    return {k: rng_tensor(v.shape, 100 + it * 7 + i) * mul for i, (k, v) in enumerate(vals.items())}


def _set_grads(store, grads):
    for k, g in grads.items():
        store.params[k]._of_grad.copy_(g.cuda())


def _moment(store, arena, name):
    o = store.offsets[name]
    return arena[o:o + store.spec[name].size].view(store.spec[name].shape)


def _norm64(grads, gscale=1.0):
    return math.sqrt(sum(float((g.double() * gscale).pow(2).sum()) for g in grads.values()))


@pytest.mark.parametrize("gscale", [1.0, 0.125])
def test_clipped_adam_vs_oracle(gscale):
    """Three steps with gradient norms N0, ~10 N0, ~N0 and global_clipnorm = 1.5 N0 (only
    step 1 clips) against the oracle's Adam fed g * min(1, c / norm) in float64: parameters,
    m and v at test_keras_adam's 1e-5 (the first Adam steps are nearly invariant to the
    gradient's scale, so the parameters alone cannot show a missing clip), last_grad_norm at
    1e-6.  Negative control: the unclipped oracle must miss the device result by > 1e-3
    somewhere, or the inputs do not exercise the clip.

    The oracle gets the betas as the device gets them: the C ABI, like TensorFlow for float32
    variables, takes beta_1 and beta_2 as float32, and 1 - float32(0.999) differs from 0.001 by
    1.29e-5 relative.  That is the whole error of v against an oracle built with the double
    0.999 (measured: rel_inf 1.2899e-05 on flow_module_3/conv0/kernel at both grad scales, while
    m and the parameters pass); test_keras_adam asserts the parameters only, which do not see
    it."""
    from optical_flow_amd.train import KerasAdam
    store, vals = _head_store()
    muls = (1.0, 10.0, 1.0)
    n0 = _norm64(_head_grads(vals, 0), gscale)
    c = 1.5 * n0
    opt = KerasAdam(store, learning_rate=1e-2, global_clipnorm=c)
    b1, b2 = float(np.float32(opt.beta_1)), float(np.float32(opt.beta_2))
    ref = R.KerasAdam(lr=1e-2, beta1=b1, beta2=b2)
    ref_unclipped = R.KerasAdam(lr=1e-2, beta1=b1, beta2=b2)
    pref = {k: torch.tensor(v, dtype=torch.float64) for k, v in vals.items()}
    punc = {k: v.clone() for k, v in pref.items()}
    clipped = []
    for it in range(3):
        grads = _head_grads(vals, it, muls[it])
        _set_grads(store, grads)
        opt.apply_gradients(grad_scale=gscale)
        norm = _norm64(grads, gscale)
        got = opt.last_grad_norm.item()
        print("step %d norm64 %.9e device %.9e clip %.9e" % (it, norm, got, c))
        assert abs(got - norm) <= 1e-6 * norm
        f = min(1.0, c / norm)
        clipped.append(f < 1.0)
        ref.step(pref, {k: g.double() * gscale * f for k, g in grads.items()})
        ref_unclipped.step(punc, {k: g.double() * gscale for k, g in grads.items()})
    assert clipped == [False, True, False]
    assert opt.iterations == 3 and opt.skipped_updates == 0
    miss = 0.0
    for k in vals:
        m, v = _moment(store, opt.m, k), _moment(store, opt.v, k)
        assert rel_inf(store.params[k], pref[k]) < 1e-5, k
        assert rel_inf(m, ref.m[k]) < 1e-5, k
        assert rel_inf(v, ref.v[k]) < 1e-5, k
        miss = max(miss, rel_inf(store.params[k], punc[k]), rel_inf(m, ref_unclipped.m[k]),
                   rel_inf(v, ref_unclipped.v[k]))
    print("unclipped reference misses by %.3e" % miss)
    assert miss > 1e-3, miss


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    """Bitwise equality, NaNs included."""
    return torch.equal(_bits(a), _bits(b))


def _run_head(kw, steps, gscale=1.0, poison=None):
    """A fresh head store and KerasAdam(**kw); steps: gradient seeds; poison: {step index:
    value} written into one element of the gradient arena after the gradients are in place.
    Returns (store, opt, snapshots of (p, m, v, iterations) after every step)."""
    from optical_flow_amd.train import KerasAdam
    store, vals = _head_store()
    opt = KerasAdam(store, learning_rate=1e-2, **kw)
    snaps = []
    for i, it in enumerate(steps):
        _set_grads(store, _head_grads(vals, it))
        if poison and i in poison:
            store.grad_arena[1] = poison[i]      # an element of the first tensor, not padding
        opt.apply_gradients(grad_scale=gscale)
        snaps.append((store.arena.clone(), opt.m.clone(), opt.v.clone(), opt.iterations))
    return store, opt, snaps


@pytest.mark.parametrize("gscale", [1.0, 0.125])
@pytest.mark.parametrize("kw", [dict(global_clipnorm=1e30), dict(track_grad_norm=True),
                                dict(skip_nonfinite=True),
                                dict(global_clipnorm=1e6, skip_nonfinite=True)],
                         ids=["huge_clip", "track", "guard", "clip_guard"])
def test_noop_is_bitwise_plain_adam(kw, gscale):
    """A threshold far above every norm, tracking alone, or the guard on clean gradients: three
    steps leave p, m and v bitwise those of the plain KerasAdam on the same gradients."""
    _, _, plain = _run_head({}, (0, 1, 2), gscale)
    _, opt, got = _run_head(kw, (0, 1, 2), gscale)
    for a, b in zip(got, plain):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        assert a[3] == b[3]
    assert opt.skipped_updates == 0 and opt.last_grad_norm.item() > 0.0


@pytest.mark.parametrize("clip", [None, 0.5], ids=["guard", "guard_clip"])
@pytest.mark.parametrize("bad", [float("inf"), float("nan"), float("-inf")],
                         ids=["inf", "nan", "-inf"])
def test_nonfinite_guard(bad, clip):
    """clean, poisoned, clean: the poisoned step leaves p, m, v and the step counter bitwise
    as they were and counts one skipped update; the third step then equals the second step of
    a run of the two clean steps alone, bitwise.  clip 0.5 is under every norm here, so the
    clean steps clip."""
    kw = dict(skip_nonfinite=True, global_clipnorm=clip)
    _, opt, got = _run_head(kw, (0, 1, 2), poison={1: bad})
    _, opt2, two = _run_head(kw, (0, 2))
    for k in range(3):
        assert torch.equal(got[1][k], got[0][k])
    assert got[0][3] == 1 and got[1][3] == 1 and got[2][3] == 2
    assert opt.skipped_updates == 1 and opt2.skipped_updates == 0
    for k in range(3):
        assert torch.equal(got[0][k], two[0][k]) and torch.equal(got[2][k], two[1][k])
    assert torch.isfinite(got[2][0]).all()
    assert opt.last_grad_norm.item() == opt2.last_grad_norm.item()


@pytest.mark.parametrize("bad", [float("inf"), float("nan"), float("-inf")],
                         ids=["inf", "nan", "-inf"])
def test_nonfinite_without_guard(bad):
    """Guard off, clipping on: the poisoned step turns every parameter to NaN, which is what
    tf.clip_by_global_norm documents.  Guard and clipping both off (tracking alone): the plain
    update, bitwise the plain KerasAdam's on the same poisoned gradients."""
    store, opt, got = _run_head(dict(global_clipnorm=0.5), (0, 1), poison={1: bad})
    assert torch.isfinite(got[0][0]).all()
    assert torch.isnan(got[1][0]).all() and got[1][3] == 2 and opt.skipped_updates == 0
    assert not math.isfinite(opt.last_grad_norm.item())
    _, _, plain = _run_head({}, (0, 1), poison={1: bad})
    _, opt, track = _run_head(dict(track_grad_norm=True), (0, 1), poison={1: bad})
    for a, b in zip(track, plain):
        assert _same(a[0], b[0]) and _same(a[1], b[1]) and _same(a[2], b[2]) and a[3] == b[3]
    assert not torch.isfinite(plain[1][0]).all()            # today's behaviour: it spreads
    assert not math.isfinite(opt.last_grad_norm.item())


# --------------------------------------------------------------------- whole step -------
def _setup(H, W, B, seed=0):
    from optical_flow_amd.data import synthetic_batch
    from optical_flow_amd.model import FlowNet
    from optical_flow_amd.params import encoder_blocks, flow_net_spec, init_params, perturb_params
    vals = perturb_params(init_params(flow_net_spec(), seed), seed + 1)
    net = FlowNet(H, W, values=vals)
    batch = synthetic_batch(B, H, W, seed=1234 + seed)
    return net, vals, batch, list(encoder_blocks())


def test_clipped_train_steps_vs_oracle():
    """Three train steps of the 64 x 128, B = 2 net with global_clipnorm = half the oracle's
    float64 step-0 global norm, against the oracle's gradients, clipped in float64, through the
    oracle's Adam: loss, last_grad_norm and the final weights at 1e-3; and the norm over the
    arena equals the norm over the gradient tensors (the arena's alignment padding is 0)."""
    from optical_flow_amd.train import KerasAdam, Trainer
    net, vals, batch, blocks = _setup(64, 128, 2, seed=3)
    p = {k: torch.tensor(v, dtype=torch.float64) for k, v in vals.items()}
    opt_o = R.KerasAdam(lr=1e-4)
    bd = dev(torch.from_numpy(batch))
    bo = torch.tensor(batch, dtype=torch.float64)
    trainer = c = None
    for step in range(3):
        lo, _, go = R.train_step(bo, p, blocks, None)
        norm = math.sqrt(sum(float(g.pow(2).sum()) for g in go.values()))
        if step == 0:
            c = 0.5 * norm
            trainer = Trainer(net, KerasAdam(net.store, learning_rate=1e-4, global_clipnorm=c))
        f = min(1.0, c / norm)
        opt_o.step(p, {k: g * f for k, g in go.items()})
        ld, _ = trainer.train_step(bd, step)
        got = trainer.optimizer.last_grad_norm.item()
        rel = abs(ld.item() - lo.item()) / abs(lo.item())
        print("step %d loss hip %.6e oracle %.6e rel %.2e; norm hip %.6e oracle %.6e clip %.6e" % (
            step, ld.item(), lo.item(), rel, got, norm, c))
        assert rel < REL_TOL
        assert abs(got - norm) < REL_TOL * norm
        tensors = math.sqrt(sum(float(g.double().pow(2).sum())
                                for g in net.store.grads().values()))
        assert abs(got - tensors) <= 1e-6 * tensors
        if step == 0:
            assert f == 0.5
    for name in net.weight_names:
        assert rel_l2(net.store.params[name], p[name]) < REL_TOL, name


# -------------------------------------------------------------------------- graph -------
def _poison_trainer(H, W, seed=3, **opt_kw):
    from optical_flow_amd.model import FlowNet
    from optical_flow_amd.params import flow_net_spec, init_params, perturb_params
    from optical_flow_amd.train import KerasAdam, Trainer

    class PoisonTrainer(Trainer):
        """train_step with a device scalar added to one gradient element between the backward
        and the update: 0 leaves the gradient as it is, inf poisons it."""

        def train_step(self, batch_imgs, step_count=0):
            store = self.flow_net.store
            store.zero_grad()
            flows = self.flow_net(batch_imgs)
            loss_value = self.loss_layer(batch_imgs, flows)
            loss_value.backward()
            k = store.numel // 2
            store.grad_arena[k:k + 1].add_(self.poison)
            self.optimizer.apply_gradients(grad_scale=1.0)
            return loss_value.detach(), [f.detach() for f in flows]

    vals = perturb_params(init_params(flow_net_spec(), seed), seed + 1)
    net = FlowNet(H, W, values=vals)
    t = PoisonTrainer(net, KerasAdam(net.store, learning_rate=1e-4, **opt_kw))
    t.poison = torch.zeros(1, device="cuda")
    return t


def _state(t):
    o = t.optimizer
    return t.flow_net.store.arena.clone(), o.m.clone(), o.v.clone()


@pytest.mark.parametrize("mode", ["guard", "clip"])
def test_graph_replays(mode):
    """The clipped / guarded update inside a captured step (deterministic mode, fp32).
    guard: replays with the poison scalar at 0, inf, 0 -- the second leaves weights, moments
    and the step counter bitwise unchanged and counts one skipped update, and after the third
    the state is bitwise that of the eager run of the same trainer.  clip: the scalar stays 0
    and the threshold is half the first step's norm; every replay equals the eager step
    bitwise."""
    from optical_flow_amd import ops
    from optical_flow_amd.data import synthetic_batch
    H, W, B = 64, 128, 2
    b0 = dev(torch.from_numpy(synthetic_batch(B, H, W, seed=7)))
    with ops.deterministic(True):
        if mode == "guard":
            kw, seq = dict(skip_nonfinite=True), (0.0, float("inf"), 0.0)
        else:
            probe = _poison_trainer(H, W, track_grad_norm=True)
            probe.train_step(b0)
            kw, seq = dict(global_clipnorm=0.5 * probe.optimizer.last_grad_norm.item()), (0.0,) * 3
        eager = _poison_trainer(H, W, **kw)
        eager.train_step(b0)                                 # the graphed trainer's warm-up step
        want = []
        for val in seq:
            eager.poison.fill_(val)
            eager.train_step(b0)
            want.append(_state(eager) + (eager.optimizer.iterations,
                                         eager.optimizer.last_grad_norm.item()))
        gt = _poison_trainer(H, W, **kw)
        step = gt.graphed(b0.clone(), warmup=1)
        got = []
        for val in seq:
            gt.poison.fill_(val)
            step(b0)
            torch.cuda.synchronize()
            got.append(_state(gt) + (gt.optimizer.iterations, gt.optimizer.last_grad_norm.item()))
    for k, (a, b) in enumerate(zip(got, want)):
        for i in range(3):
            assert torch.equal(a[i], b[i]), (k, i)
        assert a[3] == b[3], k
        assert a[4] == b[4] or (math.isinf(a[4]) and math.isinf(b[4])), (k, a[4], b[4])
    if mode == "guard":
        for i in range(3):
            assert torch.equal(got[1][i], got[0][i])
            assert not torch.equal(got[2][i], got[1][i])
        assert [g[3] for g in got] == [2, 2, 3]
        assert math.isinf(got[1][4])
        assert gt.optimizer.skipped_updates == 1 and eager.optimizer.skipped_updates == 1
    else:
        assert all(g[4] > kw["global_clipnorm"] for g in got)     # every replay clipped
        assert [g[3] for g in got] == [2, 3, 4]
        assert gt.optimizer.skipped_updates == 0


# ----------------------------------------------------------------- data parallel --------
def test_rccl_dp_world1_clipped():
    """Trainer(data_parallel=True, comm=<one-rank RCCL communicator>) with clipping: the norm
    is taken on the reduced arena after finish(), so two steps equal the plain clipped
    trainer's bitwise in deterministic mode (weights, moments, norm)."""
    from optical_flow_amd import ops
    from optical_flow_amd.comm import RcclComm
    from optical_flow_amd.train import KerasAdam, Trainer
    H, W, B = 64, 128, 2

    def run(comm, **kw):
        net, _, batch, _ = _setup(H, W, B)
        tr = Trainer(net, KerasAdam(net.store, learning_rate=1e-3, **kw),
                     data_parallel=comm is not None, comm=comm)
        x = dev(torch.from_numpy(batch))
        norms = []
        for s in range(2):
            tr.train_step(x, s)
            norms.append(tr.optimizer.last_grad_norm.item())
        torch.cuda.synchronize()
        return tr, norms

    with ops.deterministic(True):
        _, probe = run(None, track_grad_norm=True)
        kw = dict(global_clipnorm=0.5 * min(probe), skip_nonfinite=True)
        plain, n_plain = run(None, **kw)
        comm = RcclComm(0, 1)
        dp, n_dp = run(comm, **kw)
    assert dp.reducer is not None and dp.reducer.comm is comm and dp.reducer.world == 1
    assert n_dp == n_plain and n_plain[0] == probe[0]
    assert all(n > kw["global_clipnorm"] for n in n_dp)
    assert torch.equal(dp.flow_net.store.arena, plain.flow_net.store.arena)
    assert torch.equal(dp.optimizer.m, plain.optimizer.m)
    assert torch.equal(dp.optimizer.v, plain.optimizer.v)
    assert dp.optimizer.iterations == 2 and dp.optimizer.skipped_updates == 0
    comm.close()


# -------------------------------------------------------------------- train command -----
def test_train_command_logs_norm_and_skips(tmp_path):
    """python -m optical_flow_amd.train --clip-norm C --skip-nonfinite --log: a header record
    with the three settings, then per step grad_norm and skipped beside step, loss and t; a
    default run's log has neither a header nor the new keys."""
    import json
    from optical_flow_amd.train import main
    size = ["--height", "64", "--width", "64", "--batch", "1", "--steps", "2"]
    log = tmp_path / "clip.jsonl"
    main(size + ["--clip-norm", "0.05", "--skip-nonfinite", "--log", str(log)])
    recs = [json.loads(l) for l in open(log).read().splitlines() if l]
    head = recs[0]
    assert head["header"] is True and "step" not in head
    assert (head["clip_norm"], head["skip_nonfinite"], head["log_grad_norm"]) == (0.05, True, False)
    assert [r["step"] for r in recs[1:]] == [0, 1]
    for r in recs[1:]:
        assert set(r) == {"step", "loss", "t", "grad_norm", "skipped"}
        assert math.isfinite(r["grad_norm"]) and r["grad_norm"] > 0.0 and r["skipped"] == 0
    plain = tmp_path / "plain.jsonl"
    main(size + ["--log", str(plain)])
    recs = [json.loads(l) for l in open(plain).read().splitlines() if l]
    assert len(recs) == 2 and all(set(r) == {"step", "loss", "t"} for r in recs)
    tracked = tmp_path / "track.jsonl"
    main(size + ["--log-grad-norm", "--log", str(tracked)])
    recs = [json.loads(l) for l in open(tracked).read().splitlines() if l]
    assert recs[0]["clip_norm"] is None and recs[0]["log_grad_norm"] is True
    assert all("grad_norm" in r for r in recs[1:])
