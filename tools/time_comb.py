#!/usr/bin/env python3
"""Per-leapfrog time of occu_comb (re_kernel.hpp, kind 8) at the reference's default shape (100 sites, 3 + 24 + 24 replicates) and at
10 000 sites.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/time_comb.py` for the kernel's own statistics."""
import contextlib, io, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from biolith_amd.engine import OccuDataset
from biolith_amd.models import simulate_comb


def run(name, data, chains=5):
    ds = OccuDataset(data["site_covs"], data["PC_obs_covs"], data["PC_obs"], model="occu_comb", ARU_obs_covs=data["ARU_obs_covs"],
                     ARU_obs=data["ARU_obs"], scores_obs=data["scores_obs"])
    ds.nuts(num_warmup=300, num_samples=300, num_chains=chains, seed=0)   # (first launch: code-object load, allocation)
    r = ds.nuts(num_warmup=1000, num_samples=1000, num_chains=chains, seed=1)
    per_chain = r.n_leapfrog.reshape(chains, -1).sum(axis=1)
    print(f"{name:40s} D={ds.D:3d} chains={chains} k={r.wgs_per_chain} kernel {r.kernel_ms:9.2f} ms  "
          f"{1e3 * r.kernel_ms / per_chain.max():7.2f} us per leapfrog of the slowest chain  ({r.kernel_name})  "
          f"steps/transition {r.num_steps.mean():6.1f} div {r.diverging.mean():.3f}")


with contextlib.redirect_stdout(io.StringIO()):
    d_ref, _ = simulate_comb(simulate_missing=True)
    d_big, _ = simulate_comb(simulate_missing=True, n_sites=10000)
run("default: 100 sites x (3 + 24 + 24)", d_ref)
run("10 000 sites x (3 + 24 + 24)", d_big)
