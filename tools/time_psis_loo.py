"""Wall time and peak host memory of PSIS-LOO on a (draws, cells) log-likelihood matrix: the device path (engine.psis_loo, one bl_psis_loo
call) against the float64 NumPy restatement of the same definition (tests/psis_ref.py, column by column).  4000 draws x 10 000 cells,
generated as the tests generate theirs: normal(-3, 0.3) scaled per column by uniform(0.5, 2), every fourth column -log of Pareto
ratios with k0 = 0.7.

Each path runs in a fresh child process of its own, so that its peak resident set (ru_maxrss) is its own.  The device child warms up on
64 cells (code objects, first allocations), then times whole calls with a host clock -- a call uploads the matrix and ends in the copy
of the results back to the host, so the device work is inside the window.  The host child times --host-cells columns (default 500) and
scales to all of them: the figure it prints is marked as scaled.  The parent prints one JSON line.

    python tools/time_psis_loo.py [--draws 4000] [--cells 10000] [--host-cells 500] [--reps 3]"""
import argparse
import json
import os
import resource
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _matrix(n, cells):
    rng = np.random.default_rng(0)
    ll = (rng.normal(-3.0, 0.3, (n, cells)) * rng.uniform(0.5, 2.0, cells)).astype(np.float32)
    heavy = np.arange(cells) % 4 == 3
    ll[:, heavy] = (0.7 * np.log1p(-rng.uniform(size=(n, int(heavy.sum())))) - 3.0).astype(np.float32)
    return ll


def child(path, n, cells, host_cells, reps):
    ll = _matrix(n, cells)
    rss_input = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    if path == "device":
        from biolith_amd.engine import psis_loo

        psis_loo(ll[:, :64])
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            elpd, k, lppd = psis_loo(ll)
            times.append(time.perf_counter() - t0)
        out = dict(wall_s=times, cells_timed=cells, scaled=False)
    else:
        import psis_ref

        m = min(host_cells, cells)
        t0 = time.perf_counter()
        elpd, k, lppd = psis_ref.matrix(ll[:, :m])
        dt = time.perf_counter() - t0
        out = dict(wall_s=[dt * cells / m], cells_timed=m, scaled=m < cells, wall_s_timed=dt)
    out.update(path=path, elpd_sum_of_timed_cells=float(np.sum(elpd)), k_max=float(np.max(k)), k_above_07=int(np.sum(k > 0.7)),
               peak_rss_mb=resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0, rss_with_input_mb=rss_input / 1024.0)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=4000)
    ap.add_argument("--cells", type=int, default=10000)
    ap.add_argument("--host-cells", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--child", choices=["device", "host"])
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.draws, a.cells, a.host_cells, a.reps)
    runs = []
    for path in ("device", "host"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "--draws", str(a.draws), "--cells", str(a.cells),
                            "--host-cells", str(a.host_cells), "--reps", str(a.reps)], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.exit(f"{path} child failed ({r.returncode}):\n{r.stderr[-2000:]}")
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps(dict(shape=f"{a.draws} draws x {a.cells} cells", runs=runs)))


if __name__ == "__main__":
    main()
