"""Time bl_site_posterior against bl_predict (latent and y) on the same handle and draws: the headline shape (10 000 sites x 5 visits,
3 + 3 covariates, 4 000 draws) and simulate_comb(n_sites=10000) (occu_comb has no bl_predict: its line stands alone).

Prints the wall time of each call (upload of the draws, kernels, copies back).  The kernels' own times come from running this script
under the profiler:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_latent.py  (bl_site_posterior_kernel, bl_predict_kernel)."""
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from biolith_amd.engine import OccuDataset  # noqa: E402
from biolith_amd.models import simulate, simulate_comb  # noqa: E402


def best(fn, reps=3):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return min(out)


def main():
    n = 4000
    rng = np.random.default_rng(0)
    with contextlib.redirect_stdout(io.StringIO()):
        data, _ = simulate(n_sites=10000, n_site_covs=3, n_obs_covs=3, deployment_days_per_site=35, session_duration=7)
        comb, _ = simulate_comb(n_sites=10000)
    ds = OccuDataset(data["site_covs"], data["obs_covs"], data["obs"])
    th = rng.uniform(-1, 1, size=(n, ds.D)).astype(np.float32)
    res = dict(shape="10000 x 5, 3 + 3 covariates, 4000 draws")
    res["site_posterior_ms"] = best(lambda: ds.site_posterior(th, seed=1))
    res["predict_ms"] = best(lambda: ds.predictive(th, seed=1))
    res["ratio"] = res["site_posterior_ms"] / res["predict_ms"]
    ds.close()
    dc = OccuDataset(comb["site_covs"], comb["PC_obs_covs"], comb["PC_obs"], model="occu_comb", ARU_obs_covs=comb["ARU_obs_covs"],
                     ARU_obs=comb["ARU_obs"], scores_obs=comb["scores_obs"])
    thc = rng.uniform(-0.7, 0.7, size=(n, dc.D)).astype(np.float32)
    thc[:, -6:] = np.array([-1.2, -1.5, -2.0, 1.6, 1.5, 1.1]) + rng.uniform(-0.4, 0.4, size=(n, 6))
    res["comb_site_posterior_ms"] = best(lambda: dc.site_posterior(thc, seed=1))
    dc.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
