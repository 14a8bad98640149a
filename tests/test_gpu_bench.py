"""A plain `bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` at a small size: the headline leg alone, K timed steps,
one JSON line with ms_per_step, and the last step's outputs as .npy files that a second run with the same arguments reproduces."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--windows", "64", "--enc-batch", "32", "--steps", "2",
           "--warmup", "1", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_bench_run_times_the_headline_leg_and_dumps_its_outputs(dev, tmp_path):
    line = _plain_run(tmp_path / "a")
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["dtype"] == "f16x3" and line["unit"] == "clip-windows/s" and line["higher_is_better"] is True
    assert line["value"] == pytest.approx(64 * 1e3 / line["ms_per_step"], rel=1e-3)
    for moved in ("fast_mode_value", "value_inputs_r03", "precision_max_abs_dscore", "cpu_baseline", "train_clips_per_s"):
        assert moved not in line, moved
    got = {p.name[:-4]: np.load(p) for p in sorted((tmp_path / "a").iterdir())}
    assert {"rows", "select_idx", "select_cnt", "sim_rows", "q_emb_rows", "t_emb_rows"} <= set(got)
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert got["select_idx"].shape == (64, 64) and got["sim_rows"].shape == (64, 64) and got["q_emb_rows"].shape == (64, 2304)
    assert np.all(np.isfinite(got["sim_rows"])) and np.allclose(np.linalg.norm(got["q_emb_rows"], axis=1), 1.0, atol=1e-5)
    # the same arguments, the same inputs: a second process computes the same outputs
    _plain_run(tmp_path / "b")
    for name, v in got.items():
        w = np.load(tmp_path / "b" / (name + ".npy"))
        assert w.shape == v.shape and np.allclose(w, v, rtol=1e-5, atol=1e-6), name
