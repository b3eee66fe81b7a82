"""Wall time and peak host memory of the count models' posterior predictive check, fused (utils.predictive_check_counts) against the
host path (evaluation.posterior_predictive_check_counts on predict()'s arrays): nmixture, 10 000 sites x 1 period x 5 visits, 3 + 3
covariates, 1000 draws, about 10 % of the observations missing, by site, Freeman-Tukey.

Each path runs in a fresh child process of its own, so that its peak resident set (ru_maxrss) is its own; the children alternate
(fused, host, fused, host).  A child warms up on 8 draws (code objects, first allocations), then times whole calls with a host clock --
every call ends in a copy back to the host, so the device work is inside the window; the fused call is milliseconds, so it is repeated
more often (--fused-reps) than the host path (--reps).  The host path is the baseline.  The parent prints one JSON line.

    python tools/time_predictive_check_counts.py [--draws 1000] [--sites 10000] [--rounds 2]"""
import argparse
import json
import os
import resource
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MAX_ABUNDANCE = 30


class _Posterior:
    def __init__(self, sites):
        self.sites = sites

    def get_samples(self):
        return self.sites


def _case(N, n, J=5, K=3):
    rng = np.random.default_rng(0)
    data = dict(site_covs=rng.normal(size=(N, K)).astype(np.float32), obs_covs=rng.normal(size=(N, 1, J, K)).astype(np.float32))
    obs = rng.binomial(rng.poisson(2.0, (1, N, 1, 1)), 0.4, (1, N, 1, J)).astype(np.float32)
    obs[rng.random(obs.shape) < 0.1] = np.nan
    data["obs"] = obs
    sites = dict(beta=rng.uniform(-0.5, 0.5, (n, 1, K + 1)).astype(np.float32), alpha=rng.uniform(-1, 1, (n, 1, K + 1)).astype(np.float32))
    return data, sites


def child(path, N, n, reps):
    from biolith_amd.evaluation import posterior_predictive_check_counts
    from biolith_amd.models import nmixture
    from biolith_amd.utils import predict, predictive_check_counts

    data, sites = _case(N, n)

    def run(m):
        post = _Posterior({k: v[:m] for k, v in sites.items()})
        if path == "fused":
            return predictive_check_counts(nmixture, post, **data, max_abundance=MAX_ABUNDANCE, random_seed=1)["p_value"]
        preds = predict(nmixture, post, **data, max_abundance=MAX_ABUNDANCE, num_samples=m, random_seed=1)
        return posterior_predictive_check_counts(nmixture, preds, data["obs"], "site", "freeman-tukey", max_abundance=MAX_ABUNDANCE)

    run(8)
    rss_warm = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    times, res = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = run(n)
        times.append(time.perf_counter() - t0)
    rss = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    print(json.dumps(dict(path=path, p_value=res, wall_s=times, peak_rss_mb=rss / 1024.0, rss_after_warmup_mb=rss_warm / 1024.0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--sites", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--fused-reps", type=int, default=20)
    ap.add_argument("--child", choices=["fused", "host"])
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.sites, a.draws, a.reps)
    runs = []
    for _ in range(a.rounds):
        for path in ("fused", "host"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "--draws", str(a.draws), "--sites", str(a.sites),
                                "--reps", str(a.fused_reps if path == "fused" else a.reps)], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.exit(f"{path} child failed ({r.returncode}):\n{r.stderr[-2000:]}")
            runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    best = lambda path, key, f: f(f(x[key]) if isinstance(x[key], list) else x[key] for x in runs if x["path"] == path)
    out = dict(shape=f"nmixture, {a.sites} sites x 1 x 5 visits, 3 + 3 covariates, max_abundance {MAX_ABUNDANCE}, {a.draws} draws", runs=runs)
    for path in ("fused", "host"):
        out[f"{path}_wall_s_min"] = best(path, "wall_s", min)
        out[f"{path}_wall_s_max"] = best(path, "wall_s", max)
        out[f"{path}_peak_rss_mb"] = best(path, "peak_rss_mb", max)
    fused, host = (next(x["p_value"] for x in runs if x["path"] == p) for p in ("fused", "host"))
    out["p_value_fused"], out["p_value_host"], out["p_values_agree"] = fused, host, fused == host
    print(json.dumps(out))


if __name__ == "__main__":
    main()
