"""GPU test of bench.py's plain run: one JSON line with the headline fields, exactly --steps timed steps, and the fields
--dump-outputs writes are the analysis the timed path computed (float64 oracle on the same seeded month)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oisatgmi import synthetic as syn
from oracle import oi_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_dumps_the_last_step_analysis(tmp_path):
    import bench
    wl = "config1_72x144_1e3obs"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--workload", wl, "--dump-outputs", str(tmp_path)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["unit"] == "grid-cells/s" and out["dtype"] == "f32"
    assert out["higher_is_better"] is True and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(72 * 144 / (out["ms_per_step"] * 1e-3), rel=1e-9)
    for key in ("roofline", "secondary", "tiled", "config4_strong", "cpu_baseline"):
        assert key not in out, key                       # --full only
    xa, inc = np.load(tmp_path / "xa.npy"), np.load(tmp_path / "inc.npy")
    assert xa.dtype == np.float32 and xa.shape == (72, 144) and inc.shape == (72, 144)
    ny, nx, nobs, L, _, _ = bench.WORKLOADS[wl]
    lat2, lon2 = syn.global_grid(ny, nx)
    p, cell, _, _ = bench.build_case(wl, 4000, lat2, lon2)
    want = orc.dense_oi(lat2, lon2, p.Xa, p.Sa, p.obs_lat, p.obs_lon, cell, np.where(p.obs_y < 0, 0, p.obs_y), p.obs_var, L)
    scale = np.abs(want["xa"]).max()
    assert np.abs(xa.ravel() - want["xa"]).max() <= 1e-5 * scale
    assert np.abs(inc.ravel() - want["inc"]).max() <= 1e-5 * scale
