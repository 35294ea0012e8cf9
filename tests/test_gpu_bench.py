"""bench.py end to end at a small size, in a process of its own like its callers run it: the
plain run (headline figure only, --dump-outputs) and the --full run (roofline, CPU baseline,
parity) print one JSON line with the contract fields."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, B = 64, 128, 1
SMALL = ["--gpus", "1", "--height", str(H), "--width", str(W), "--batch", str(B)]


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + list(args),
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _check_contract(out, steps, warmup):
    assert out["metric"] == "image-pairs/sec training, %dx%d batch=%d per GPU" % (H, W, B)
    assert out["unit"] == "image-pairs/s" and out["higher_is_better"] is True
    assert out["dtype"] == "fp32" and out["n_gpus"] == 1
    assert out["steps"] == steps and out["warmup"] == warmup
    assert out["value"] > 0 and out["ms_per_step"] > 0
    # value and ms_per_step describe the same timed region of `steps` steps (both are rounded
    # to 3 decimals in the line)
    assert abs(out["value"] * out["ms_per_step"] / (1e3 * B) - 1) < 1e-2


def test_bench_plain_line_and_dump(tmp_path):
    """The plain run measures the headline figure only, and --dump-outputs writes what the
    last timed step returned: the loss the line reports and the four flows (float32)."""
    d = tmp_path / "out"
    out = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(d))
    _check_contract(out, 3, 1)
    assert out["full"] is False
    for k in ("roofline", "cpu_baseline", "parity", "conv_ms_per_step"):
        assert out[k] is None, k
    assert out["timed_state"]["train_steps_before_first"] == 1     # the warm-up, nothing else
    assert sorted(os.listdir(d)) == ["flow0.npy", "flow1.npy", "flow2.npy", "flow3.npy",
                                     "loss.npy"]
    loss = np.load(d / "loss.npy")
    assert loss.dtype == np.float32 and loss.shape == (1,)
    assert float(loss[0]) == out["final_loss"]
    for i in range(4):
        f = np.load(d / ("flow%d.npy" % i))
        assert f.dtype == np.float32 and f.shape == (B, H >> (i + 1), W >> (i + 1), 2)
        assert np.isfinite(f).all()
        # the line's mean |flow| of the last timed step (float32 mean, rounded to 4 decimals)
        want = out["timed_state"]["last"]["flow_abs_mean"][i]
        assert abs(np.abs(f).mean(dtype=np.float64) - want) <= 1e-4 + 1e-5 * want


def test_bench_full_line():
    """--full keeps the whole line: the dominant kernel's roofline with its per-kernel tables,
    the CPU baseline and the parity of the HIP path against the oracle."""
    out = _bench("--full", "--steps", "3", "--warmup", "1", "--cpu-steps", "1")
    _check_contract(out, 3, 1)
    assert out["full"] is True
    assert out["timed_state"]["train_steps_before_first"] == 3     # warm-up + 2 profiled steps
    roof = out["roofline"]
    assert roof["achieved"] > 0 and roof["per_kernel"] and roof["per_kernel_alone"]
    assert out["conv_ms_per_step"] > 0
    assert out["cpu_baseline"]["value"] > 0
    assert max(out["parity"]["flow_rel_inf"]) < 1e-3 and out["parity"]["loss_rel"] < 1e-3
    assert max(out["parity"]["final_weights"]["flow_rel_inf"]) < 1e-3
