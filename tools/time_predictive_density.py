"""Wall time and peak host memory of WAIC, lppd and deviance, fused (utils.information_criteria) against the host path
(evaluation.waic and evaluation.deviance on predict()'s arrays): 10 000 sites x 1 period x 5 visits, 3 + 3 covariates, 1000 draws, about
10 % of the observations missing, the conditional form.

Each path runs in a fresh child process of its own, so that its peak resident set (ru_maxrss) is its own; the children alternate
(fused, host, fused, host).  A child warms up on 8 draws (code objects, first allocations), then times whole calls with a host clock --
every call ends in a copy back to the host, so the device work is inside the window.  The parent prints one JSON line.

    python tools/time_predictive_density.py [--draws 1000] [--sites 10000] [--rounds 2]"""
import argparse
import json
import os
import resource
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class _Posterior:
    def __init__(self, sites):
        self.sites = sites

    def get_samples(self):
        return self.sites


def _case(N, n, J=5, K=3):
    rng = np.random.default_rng(0)
    data = dict(site_covs=rng.normal(size=(N, K)).astype(np.float32), obs_covs=rng.normal(size=(N, 1, J, K)).astype(np.float32))
    obs = (rng.random((1, N, 1, J)) < 0.3).astype(np.float32)
    obs[rng.random(obs.shape) < 0.1] = np.nan
    data["obs"] = obs
    sites = dict(beta=rng.uniform(-1, 1, (n, 1, K + 1)).astype(np.float32), alpha=rng.uniform(-1, 1, (n, 1, K + 1)).astype(np.float32))
    return data, sites


def child(path, N, n, reps):
    from biolith_amd.evaluation import deviance, waic
    from biolith_amd.models import occu
    from biolith_amd.utils import information_criteria, predict

    data, sites = _case(N, n)

    def run(m):
        post = _Posterior({k: v[:m] for k, v in sites.items()})
        if path == "fused":
            ic = information_criteria(occu, post, **data, random_seed=1)
            return {k: ic[k] for k in ("waic", "lppd", "p_waic", "deviance")}
        preds = predict(occu, post, **data, num_samples=m, random_seed=1)
        return {**waic(occu, preds, **data), "deviance": deviance(occu, preds, **data)}

    run(8)
    rss_warm = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    times, res = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = run(n)
        times.append(time.perf_counter() - t0)
    rss = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    print(json.dumps(dict(path=path, result=res, wall_s=times, peak_rss_mb=rss / 1024.0, rss_after_warmup_mb=rss_warm / 1024.0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--sites", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--child", choices=["fused", "host"])
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.sites, a.draws, a.reps)
    runs = []
    for _ in range(a.rounds):
        for path in ("fused", "host"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "--draws", str(a.draws), "--sites", str(a.sites),
                                "--reps", str(a.reps)], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.exit(f"{path} child failed ({r.returncode}):\n{r.stderr[-2000:]}")
            runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    best = lambda path, key, f: f(f(x[key]) if isinstance(x[key], list) else x[key] for x in runs if x["path"] == path)
    out = dict(shape=f"{a.sites} sites x 1 x 5 visits, 3 + 3 covariates, {a.draws} draws", runs=runs)
    for path in ("fused", "host"):
        out[f"{path}_wall_s_min"] = best(path, "wall_s", min)
        out[f"{path}_peak_rss_mb"] = best(path, "peak_rss_mb", max)
    fused, host = (next(x["result"] for x in runs if x["path"] == p) for p in ("fused", "host"))
    out["largest_relative_difference"] = max(abs(fused[k] - host[k]) / abs(host[k]) for k in host)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
