"""bench.py on the GPU, the way every change is measured: a plain run times exactly --steps steps, prints ONE JSON line with the
headline keys and none of the --full measurements, and --dump-outputs writes float32 / float64 .npy files of the last timed step
(2 decoder layers here: the line is then marked INVALID, the path is the same)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_dumps_outputs(tmp_path):
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--layers", "2",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "pairs/s" and line["dtype"] == "bf16" and line["higher_is_better"]
    assert line["ms_per_step"] > 0 and abs(line["value"] - 4 * 1e3 / line["ms_per_step"]) / line["value"] < 0.01
    assert not {"roofline", "cpu_baseline", "variants"} & set(line)
    files = sorted(os.listdir(out))
    arrays = {f[:-4]: np.load(out / f) for f in files}
    assert all(f.endswith(".npy") for f in files) and {"loss", "grad_norm", "master", "grads"} <= set(arrays)
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert np.isfinite(arrays["loss"]).all() and abs(float(arrays["loss"][0]) - line["config"]["loss_last_step"]) < 1e-6
    assert np.isfinite(arrays["master"]).all() and np.abs(arrays["grads"]).max() > 0
