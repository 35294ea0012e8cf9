"""Global-norm clipping and the non-finite guard, the host side (no GPU): KerasAdam's argument
validation, the train command's flags, of_grad_sumsq_partials as a pure function of n, and every
refusal of of_grad_sumsq / of_adam_keras_dev_clip, which must come back as OF_EINVAL with a
message before anything is launched (the pointers here are host buffers)."""
import ctypes as C
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from optical_flow_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def _cpu_store():
    from optical_flow_amd.model import ParamStore
    from optical_flow_amd.params import head_spec, init_params
    spec = head_spec(3)
    return ParamStore(spec, init_params(spec, 3), device="cpu")


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("inf"), float("-inf"), float("nan")])
def test_global_clipnorm_refused(lib, bad):
    from optical_flow_amd.train import KerasAdam
    with pytest.raises(ValueError, match="global_clipnorm"):
        KerasAdam.check_global_clipnorm(bad)
    store = _cpu_store()
    with pytest.raises(ValueError, match="global_clipnorm"):
        KerasAdam(store, global_clipnorm=bad)
    opt = KerasAdam(store, global_clipnorm=2.0)
    with pytest.raises(ValueError, match="global_clipnorm"):
        opt.global_clipnorm = bad
    assert opt.global_clipnorm == 2.0


def test_keras_adam_arguments(lib):
    from optical_flow_amd.train import KerasAdam
    store = _cpu_store()
    plain = KerasAdam(store)
    assert plain.global_clipnorm is None and not plain.skip_nonfinite
    assert not plain.track_grad_norm and not plain._clip_path()
    with pytest.raises(RuntimeError, match="no gradient norm"):
        plain.last_grad_norm
    with pytest.raises(RuntimeError, match="no gradient norm"):
        plain.skipped_updates
    for kw in (dict(global_clipnorm=0.5), dict(skip_nonfinite=True), dict(track_grad_norm=True)):
        opt = KerasAdam(store, **kw)
        assert opt._clip_path()
        assert opt._partials.numel() == lib.of_grad_sumsq_partials(store.numel)
        assert opt._state.numel() * 8 == lib.of_adam_clip_state_bytes()
        assert opt.last_grad_norm.dim() == 0 and float(opt.last_grad_norm) == 0.0
        assert opt.skipped_updates == 0
    opt = KerasAdam(store, global_clipnorm=3)
    assert opt.global_clipnorm == 3.0
    opt.global_clipnorm = 0.25                     # settable between steps, as learning_rate
    assert opt.global_clipnorm == 0.25
    opt.global_clipnorm = None
    assert opt.global_clipnorm is None


def test_parser_flags():
    from optical_flow_amd.train import build_parser
    ap = build_parser()
    a = ap.parse_args([])
    assert a.clip_norm is None and not a.skip_nonfinite and not a.log_grad_norm
    a = ap.parse_args(["--clip-norm", "2.5", "--skip-nonfinite", "--log-grad-norm"])
    assert a.clip_norm == 2.5 and a.skip_nonfinite and a.log_grad_norm
    a = ap.parse_args(["--skip-nonfinite"])
    assert a.clip_norm is None and a.skip_nonfinite and not a.log_grad_norm


def test_train_command_refuses_bad_clip_norm(capsys):
    from optical_flow_amd.train import main
    for bad in ("0", "-1", "nan", "inf"):
        with pytest.raises(SystemExit):
            main(["--clip-norm", bad])
        assert "--clip-norm" in capsys.readouterr().err


def test_partials_pure_function_of_n(lib):
    sizes = [0, 1, 3, 4, 5, 1023, 1024, 1025, 65535, 65536, 1 << 20, (1 << 20) + 1, 4937219,
             4937220, 1 << 22, (1 << 22) + 1, 1 << 31, (1 << 40) + 3]
    first = [lib.of_grad_sumsq_partials(n) for n in sizes]
    assert all(p >= 1 for p in first)
    assert first == [lib.of_grad_sumsq_partials(n) for n in sizes]
    assert first == sorted(first)                  # more data never means fewer workgroups
    assert lib.of_grad_sumsq_partials(-5) >= 1     # no launch geometry of 0 for a refused n


def _host(nbytes, align=16):
    raw = (C.c_char * (nbytes + 64))()
    base = C.addressof(raw)
    return raw, base + (-base) % align


N = 1000


def _sumsq_args(lib):
    keep = [_host(4 * N), _host(8 * lib.of_grad_sumsq_partials(N))]
    return keep, dict(g=keep[0][1], n=N, partials=keep[1][1])


@pytest.mark.parametrize("bad,msg", [(dict(g=None), b"null"), (dict(partials=None), b"null"),
                                     (dict(n=-1), b"n < 0"), (dict(g_off=4), b"aligned"),
                                     (dict(g_off=8), b"aligned")],
                         ids=["g_null", "partials_null", "n_negative", "g_off4", "g_off8"])
def test_grad_sumsq_refusals(lib, bad, msg):
    from optical_flow_amd._lib import OF_EINVAL
    keep, a = _sumsq_args(lib)
    off = bad.pop("g_off", 0)
    a.update(bad)
    g = a["g"] + off if a["g"] is not None else None
    st = lib.of_grad_sumsq(g, a["n"], a["partials"], None)
    assert st == OF_EINVAL, (st, lib.of_last_error())
    assert msg in lib.of_last_error().lower(), lib.of_last_error()


_ARENAS = ("p", "g", "m", "v")


@pytest.mark.parametrize("bad,msg", [(dict([(k, None)]), b"null") for k in
                                     _ARENAS + ("sched", "iter", "partials", "state")] +
                         [(dict(n=-1), b"n < 0")] +
                         [(dict([(k + "_off", 4)]), b"aligned") for k in _ARENAS] +
                         [(dict(np_delta=1), b"npartials"), (dict(np_delta=-1), b"npartials"),
                          (dict(np_zero=True), b"npartials"),
                          (dict(clip_norm=-1.0), b"clip_norm"),
                          (dict(clip_norm=float("nan")), b"clip_norm"),
                          (dict(clip_norm=float("-inf")), b"clip_norm")],
                         ids=lambda v: None if isinstance(v, bytes) else
                         ",".join("%s=%s" % kv for kv in v.items()))
def test_adam_clip_refusals(lib, bad, msg):
    from optical_flow_amd._lib import OF_EINVAL
    P = lib.of_grad_sumsq_partials(N)
    keep = {k: _host(4 * N) for k in _ARENAS}
    keep.update(sched=_host(8), iter=_host(4), partials=_host(8 * P),
                state=_host(lib.of_adam_clip_state_bytes()))
    a = {k: v[1] for k, v in keep.items()}
    a.update(n=N, np=P, clip_norm=1.0)
    for k in _ARENAS:
        a[k] += bad.pop(k + "_off", 0)
    a["np"] += bad.pop("np_delta", 0)
    if bad.pop("np_zero", False):
        a["np"] = 0
    a.update(bad)
    st = lib.of_adam_keras_dev_clip(a["p"], a["g"], a["m"], a["v"], a["n"], a["sched"], a["iter"],
                                    0.9, 0.999, 1e-7, 1.0, a["partials"], a["np"],
                                    a["clip_norm"], 1, a["state"], None)
    assert st == OF_EINVAL, (st, lib.of_last_error())
    assert msg in lib.of_last_error().lower(), lib.of_last_error()
