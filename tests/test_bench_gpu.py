"""bench.py's plain run on the device: the result line, exactly --steps timed steps, nothing measured beside them
(no bench_extra.json), and --dump-outputs — the last timed step's loss, parameters and gradients as fp32 .npy files,
the same from run to run on the same inputs."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _run(tmp_path, tag):
    out = tmp_path / tag
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["CREAM_BENCH_EXTRA"] = str(tmp_path / f"{tag}_extra.json")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8",
           "--dump-outputs", str(out)]
    p = subprocess.run(cmd, env=env, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stderr[-3000:]}"
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert not os.path.exists(env["CREAM_BENCH_EXTRA"]), "a plain run writes no side measurements"
    return line, {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(str(out / "*.npy"))}


def test_plain_run_and_dumped_outputs(tmp_path):
    line, outs = _run(tmp_path, "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "images/sec" and line["higher_is_better"] is True
    assert line["value"] > 0 and abs(line["value"] - 8 * 1e3 / line["ms_per_step"]) <= 1e-2 * line["value"]
    assert line["roofline"] is None and line["cpu_baseline"] is None and "extra" not in line
    assert "loss" in outs and np.isfinite(outs["loss"]).all()
    assert any(k.startswith("param.") for k in outs) and any(k.startswith("grad.") for k in outs)
    assert all(v.dtype in (np.float32, np.float64) for v in outs.values())
    assert sum(v.nbytes for v in outs.values()) <= 64 << 20
    assert all(np.isfinite(v).all() for v in outs.values())
    # same arguments, same inputs: a second run hands back the same arrays
    _, again = _run(tmp_path, "b")
    assert sorted(again) == sorted(outs)
    for k, v in outs.items():
        np.testing.assert_array_equal(again[k], v, err_msg=k)
