"""bench.py's plain run (`--gpus 1 --steps N --warmup W`): only the timed steps and the result line --
no census, roofline probe, decode or CPU baseline, which belong to `--full` -- and `--dump-outputs`:
what the last timed step computed as float32 .npy files, within 64 MB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(out)]
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["n_gpus"] == 1
    assert res["unit"] == "tokens/s" and res["higher_is_better"] is True and res["dtype"] == "bf16"
    assert res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(64 * 256 / (res["ms_per_step"] * 1e-3), rel=1e-3)
    # what --full adds is absent from a plain run
    assert res["roofline"] is None
    assert not {"gemm_census_ms", "kernel_census", "generate_c5", "cpu_baseline"} & set(res)
    assert "in-step probe" not in r.stderr and "cpu baseline" not in r.stderr
    files = sorted(p.name for p in out.iterdir())
    assert files == ["grads.npy", "loss.npy", "params.npy"]
    arrs = {f[:-4]: np.load(out / f) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64_000_000
    assert arrs["loss"].shape == (1,) and round(float(arrs["loss"][0]), 4) == res["final_loss"]
    assert arrs["params"].shape == arrs["grads"].shape and arrs["params"].ndim == 1
    assert np.count_nonzero(arrs["grads"]) > arrs["grads"].size // 2
