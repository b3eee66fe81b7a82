"""Time bl_path_posterior at BASELINE.json configs[4]'s shape (2 000 sites x 8 seasons x 4 visits, 3 + 3 covariates) with 1 000 draws.

Prints the wall time of the call (upload of the draws, kernel, copies back) and the bytes the kernel writes.  The kernel's own time
comes from running this script under the profiler:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_dynamics.py
(bl_path_posterior_kernel)."""
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from biolith_amd.engine import OccuDataset  # noqa: E402
from biolith_amd.models import simulate_dyn  # noqa: E402


def main():
    n = 1000
    with contextlib.redirect_stdout(io.StringIO()):
        data, truth = simulate_dyn(n_sites=2000, n_periods=8, n_site_covs=3, n_obs_covs=3, deployment_days_per_site=28, session_duration=7)
    ds = OccuDataset(data["site_covs"], data["obs_covs"], data["obs"], model="occu_dyn")
    centre = np.concatenate([truth["beta"][0], truth["beta_col"][0], truth["beta_ext"][0], truth["alpha"][0]])
    th = (centre + np.random.default_rng(0).normal(scale=0.1, size=(n, ds.D))).astype(np.float32)
    times = []
    for _ in range(4):   # (the first call loads the code object)
        t0 = time.perf_counter()
        out = ds.path_posterior(th, seed=1)
        times.append((time.perf_counter() - t0) * 1e3)
    N, T = ds.N, ds.T
    written = n * N * (4 + 4 * T + 2 * 4 * (T - 1) + T)   # log_lik, z_prob, col_prob + ext_prob, z
    workspace = 2 * n * N * T * 4                          # the filtered log-odds: written by the forward pass, read by the backward pass
    print(json.dumps(dict(shape=f"{N} x {T} x {ds.J}, 3 + 3 covariates, {n} draws", path_posterior_ms=min(times[1:]), first_call_ms=times[0],
                          output_bytes=written, workspace_bytes=workspace, mean_z_prob=float(out[1].mean()))))
    ds.close()


if __name__ == "__main__":
    main()
