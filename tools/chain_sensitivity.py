"""profiling aid: what a microsecond of the chain's step is worth in the task-graph launch of the headline analysis.

The -DOISAT_TEST_HOOKS build of the library (liboisat_hip_testhooks.so) knows OISAT_DAG_FLAGS=512: every chain step sleeps
~5 us in front of its diagonal block (4 x s_sleep 47 = 12 032 clocks), nothing else changes.  The analysis step is timed
three times with the flag and three times without, alternating, every run a process of its own under its own time limit;
the only kernel that differs is the factor launch, so the difference of the steps is the difference of the launches.
    sensitivity = (step with - step without) / (block rows x 5 us)        1 = the launch is its chain, 0 = the chain has slack
usage: python tools/chain_sensitivity.py [M]              (default 100000 observations, 720 x 1440, L = 300 km)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oi-sat-gmi_amd")]
SLEEP_US = 4 * 47 * 64 / 2400.0                                 # at 2.4 GHz


def child(m, steps=8, warmup=2):
    import numpy as np
    from oisatgmi import _hip, dense, synthetic as syn
    ctx = _hip.Context(0, lib=_hip.load_test_hooks_library())
    ny, nx = (360, 720) if m <= 20000 else (720, 1440)
    p = syn.point_obs_case(ny, nx, m, 4000, swaths=m > 20000)
    cell = dense.regular_grid_cell(p.lat, p.lon, p.obs_lat, p.obs_lon)
    plan = dense.DenseAnalysis(p.lat, p.lon, max_obs=m, dtype=np.float32, ctx=ctx)
    plan.load_background(p.Xa, p.Sa)
    plan.load_obs(p.obs_lat, p.obs_lon, cell, np.where(p.obs_y < 0, 0, p.obs_y), p.obs_var)
    L = 500.0 if m <= 20000 else 300.0
    ms = []
    for k in range(warmup + steps):
        t0 = time.perf_counter()
        plan.run(L, refine=2)
        plan.check()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"flags": os.environ.get("OISAT_DAG_FLAGS", "0"), "block_rows": int(plan.mp // 128), "step_ms": sorted(ms)}))


def main():
    m = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    runs = {"0": [], "512": []}
    rows = None
    for flags in ("0", "512") * 3:
        env = dict(os.environ)
        env["OISAT_DAG_FLAGS"] = flags
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(m)], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.exit("run with OISAT_DAG_FLAGS=%s ended with %d: nothing more is started\n%s" % (flags, r.returncode, r.stderr[-2000:]))
        line = json.loads(r.stdout.strip().splitlines()[-1])
        rows = line["block_rows"]
        med = line["step_ms"][len(line["step_ms"]) // 2]
        runs[flags].append(med)
        print("OISAT_DAG_FLAGS=%-3s median step %.3f ms (min %.3f, max %.3f)" % (flags, med, line["step_ms"][0], line["step_ms"][-1]), flush=True)
    a, b = sorted(runs["0"])[1], sorted(runs["512"])[1]
    print("without %.3f ms, with %.3f ms: + %.3f ms for %d steps x %.2f us = %.3f ms of sleep -> sensitivity %.2f (%.3f ms of launch per us of chain step)"
          % (a, b, b - a, rows, SLEEP_US, rows * SLEEP_US * 1e-3, (b - a) / (rows * SLEEP_US * 1e-3), (b - a) / SLEEP_US))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(int(sys.argv[2]))
    else:
        main()
