"""bench.py's contract (run on an MI355X: -m gpu): a plain run prints only the headline line, --steps sets the timed steps, and
--dump-outputs writes the last timed step's arrays from inputs that are the same on every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], cwd=ROOT, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_bench_plain_run_and_dump_outputs(tmp_path):
    runs = []
    for k in range(2):
        line = _bench("--config", "c1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / f"d{k}"))
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in line, key
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert not {"roofline", "other_configs", "eager_gpu", "cpu_baseline"} & set(line), "a plain run ran a --full leg"
        runs.append({f[:-4]: np.load(tmp_path / f"d{k}" / f) for f in sorted(os.listdir(tmp_path / f"d{k}"))})
    a, b = runs
    assert a.keys() == b.keys() and {"loss", "grad_norm"} <= a.keys()
    assert any(n.startswith("param.") for n in a) and any(n.startswith("buffer.") for n in a)
    assert sum(os.path.getsize(tmp_path / "d0" / f) for f in os.listdir(tmp_path / "d0")) <= 64 * 2 ** 20
    for n in a:
        assert a[n].dtype == np.float32 and np.isfinite(a[n]).all(), n
        np.testing.assert_allclose(a[n], b[n], rtol=1e-3, atol=1e-5, err_msg=n)
