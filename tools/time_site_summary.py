"""Wall time and peak host memory of the deterministic sites' summary, fused (utils.site_summary) against the host path (predict(), then
mean, std(ddof=1) and quantile over the draw axis of both sites): occu, 10 000 sites x 1 period x 5 visits, 3 + 3 covariates, 1000 draws,
probs (0.05, 0.5, 0.95).

Time: both paths in ONE process, after a warm-up call of each at the full size, alternating (host, fused, host, fused, ...), a host
clock around whole calls -- every call ends in a copy back to the host, so the device work is inside the window.  The largest error of
the fused result against the host path's is printed as a fraction of each bound of tests/summary_ref.py.
Memory: each path once more in a fresh child process of its own (warm-up on 8 draws), so that its peak resident set is its own: VmHWM
of /proc/self/status, which starts anew at exec (ru_maxrss does not: a child inherits the high-water mark of the parent that timed the
host path).  The parent prints one JSON line.

    python tools/time_site_summary.py [--draws 1000] [--sites 10000] [--rounds 3]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_site_summary.py --kernels     # one fused call after a warm-up call"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PROBS = (0.05, 0.5, 0.95)
SITES = ("psi", "prob_detection")


class _Posterior:
    def __init__(self, sites):
        self.sites = sites

    def get_samples(self):
        return self.sites


def _case(N, n, J=5, K=3):
    rng = np.random.default_rng(0)
    data = dict(site_covs=rng.normal(size=(N, K)).astype(np.float32), obs_covs=rng.normal(size=(N, 1, J, K)).astype(np.float32))
    sites = dict(beta=rng.uniform(-1, 1, (n, 1, K + 1)).astype(np.float32), alpha=rng.uniform(-1, 1, (n, 1, K + 1)).astype(np.float32))
    return data, sites


def _paths(N, n):
    from biolith_amd.models import occu
    from biolith_amd.utils import predict, site_summary

    data, sites = _case(N, n)

    def fused(m=n):
        return site_summary(occu, _Posterior({k: v[:m] for k, v in sites.items()}), **data, probs=PROBS)

    def host(m=n):
        preds = predict(occu, _Posterior({k: v[:m] for k, v in sites.items()}), **data, num_samples=m)
        out = {}
        for name in SITES:
            v = np.asarray(preds[name]).astype(np.float64)
            out[name] = dict(mean=v.mean(0), sd=v.std(0, ddof=1), quantiles=np.quantile(v, PROBS, axis=0))
        return out

    return dict(fused=fused, host=host)


def _errors(fused, host):
    """The largest |fused - host| as a fraction of each bound of tests/summary_ref.py, over both sites."""
    worst = dict(mean=0.0, sd=0.0, quantiles=0.0)
    for name in SITES:
        f, h = fused[name], host[name]
        bound = dict(mean=1e-12 * np.abs(h["mean"]), sd=1e-10 * h["sd"] + 1e-14 * np.maximum(1.0, np.abs(h["mean"])),
                     quantiles=2e-15 * np.maximum(1.0, np.abs(h["quantiles"])))
        for k in worst:
            worst[k] = max(worst[k], float(np.max(np.abs(f[k] - h[k]) / bound[k])))
    return worst


def _peak_rss_mb():
    with open("/proc/self/status") as f:
        return next(int(line.split()[1]) for line in f if line.startswith("VmHWM:")) / 1024.0


def child(path, N, n):
    run = _paths(N, n)[path]
    run(8)
    rss_warm = _peak_rss_mb()
    t0 = time.perf_counter()
    run()
    wall = time.perf_counter() - t0
    print(json.dumps(dict(path=path, wall_s=wall, peak_rss_mb=_peak_rss_mb(), rss_after_warmup_mb=rss_warm)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--sites", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", choices=["fused", "host"])
    ap.add_argument("--kernels", action="store_true", help="a warm-up call and one fused call, nothing else (for a kernel trace)")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.sites, a.draws)
    paths = _paths(a.sites, a.draws)
    if a.kernels:
        paths["fused"](8)
        paths["fused"]()
        return
    last = {k: paths[k]() for k in ("host", "fused")}   # the warm-up call of each
    wall = dict(host=[], fused=[])
    for _ in range(a.rounds):
        for k in ("host", "fused"):
            t0 = time.perf_counter()
            last[k] = paths[k]()
            wall[k].append(time.perf_counter() - t0)
    out = dict(shape=f"occu, {a.sites} sites x 1 x 5 visits, 3 + 3 covariates, {a.draws} draws, probs {PROBS}", wall_s=wall,
               host_wall_s_min=min(wall["host"]), fused_wall_s_min=min(wall["fused"]),
               error_as_fraction_of_bound=_errors(last["fused"], last["host"]))
    del last
    for k in ("fused", "host"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", k, "--draws", str(a.draws), "--sites", str(a.sites)],
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.exit(f"{k} child failed ({r.returncode}):\n{r.stderr[-2000:]}")
        out[f"{k}_child"] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
