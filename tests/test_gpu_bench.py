"""GPU: a plain `bench.py` run is lean and shows its work.  It prints the headline line with `ms_per_step` for exactly --steps
timed steps, none of the --full measurements, and with --dump-outputs writes what its last timed step computed - identical in
two runs with the same arguments (seeded inputs, a bit-reproducible step)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "8", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir), *extra], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_plain_bench_line_and_dumped_outputs_repeat(tmp_path):
    a, b = _bench(tmp_path / "a"), _bench(tmp_path / "b")
    for line in (a, b):
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["unit"] == "images/sec" and line["higher_is_better"] is True and line["dtype"] == "bf16"
        assert not {"roofline", "kernels", "cpu_baseline", "max_px_err", "hrnet_step"} & set(line), sorted(line)
    files = sorted(os.listdir(tmp_path / "a"))
    assert {"pose.npy", "xyz_fk.npy", "loss.npy", "params.npy", "grads.npy"} <= set(files), files
    assert files == sorted(os.listdir(tmp_path / "b"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all(), f
        assert np.array_equal(x, y), f"{f}: two runs with the same arguments differ"
    assert np.load(tmp_path / "a" / "pose.npy").shape == (8, 8)
