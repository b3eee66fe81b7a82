"""Time bl_abundance_posterior against the predictive kernel of the same handle and draws (bl_predict for occu_rn, bl_predict_counts for
nmixture; latent and y): occu_rn at 5 000 sites x 10 visits (BASELINE.json configs[3]) and simulate_nmixture's defaults at 5 000 sites,
max_abundance 100, 4 000 draws around the simulator's truth.

Prints the wall time of each call (upload of the draws, kernels, copies back) and the terms per cell (visits x (max_abundance + 1)).
The kernels' own times come from running this script under the profiler:
rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_abundance.py  (bl_abundance_posterior_kernel, bl_predict_kernel,
bl_predict_counts_kernel)."""
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from biolith_amd.engine import OccuDataset  # noqa: E402
from biolith_amd.models import simulate_nmixture, simulate_rn  # noqa: E402


def best(fn, reps=3):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return min(out)


def main():
    n, K = 4000, 100
    rng = np.random.default_rng(0)
    with contextlib.redirect_stdout(io.StringIO()):
        rn, rn_truth = simulate_rn(n_sites=5000, deployment_days_per_site=70, session_duration=7)
        nm, nm_truth = simulate_nmixture(n_sites=5000)
    res = {}
    for name, data, truth in (("occu_rn", rn, rn_truth), ("nmixture", nm, nm_truth)):
        ds = OccuDataset(data["site_covs"], data["obs_covs"], data["obs"], model=name, max_abundance=K)
        center = np.r_[np.asarray(truth["beta"]).reshape(-1), np.asarray(truth["alpha"]).reshape(-1)]
        th = (center + rng.normal(scale=0.1, size=(n, ds.D))).astype(np.float32)
        r = dict(shape=f"{ds.N} x {ds.J}, max_abundance {K}, {n} draws", terms_per_cell=ds.J * (K + 1))
        r["abundance_posterior_ms"] = best(lambda: ds.abundance_posterior(th, seed=1))
        r["predict_ms"] = best(lambda: ds.predictive(th, seed=1))
        r["ratio"] = r["abundance_posterior_ms"] / r["predict_ms"]
        res[name] = r
        ds.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
