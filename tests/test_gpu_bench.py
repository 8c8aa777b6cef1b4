"""GPU (run with `-m gpu`): a plain one-GPU `bench.py` line on a small grid — `--steps` sets the Newton iterations of the timed window, the legs
beside the headline figure stay out of it without --full, and --dump-outputs writes the state the timed steps end in."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MISTARK_BENCH_DEVICE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    return json.loads(lines[0])


def test_plain_line_times_the_steps_asked_for_and_dumps_the_end_state(tmp_path):
    args = ["--gpus", "1", "--steps", "6", "--warmup", "2", "--grid", "12,12,12"]
    out = _line(args + ["--dump-outputs", str(tmp_path / "a")])
    assert out["steps"] == out["newton_iterations"] == 6 and out["warmup"] == 2
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(1e3 / out["ms_per_step"], rel=1e-9)
    assert out["metric"] == out["unit"] == "Newton-steps/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["value_windows"] is None and out["cpu_baseline"]["value"] is None and out["roofline"]["live"]["back_to_back"]["launch_ms"] is None
    x, v, box = (np.load(tmp_path / "a" / (k + ".npy")) for k in ("x", "v", "box_state"))
    assert x.dtype == v.dtype == box.dtype == np.float64 and x.shape == v.shape == (13 ** 3 + 12 ** 3, 3) and box.shape == (13,)
    assert np.isfinite(x).all() and np.isfinite(v).all() and np.abs(v).max() > 0
    # the same arguments: the same inputs, and the deterministic engine ends in the same state
    _line(args + ["--dump-outputs", str(tmp_path / "b")])
    for k in ("x", "v", "box_state"):
        assert (np.load(tmp_path / "a" / (k + ".npy")) == np.load(tmp_path / "b" / (k + ".npy"))).all(), k
