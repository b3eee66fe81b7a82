"""Wall time of the response curves, fused (utils.response_curves) against the routes that existed before them, on the same inputs:
occu, 3 site covariates, 4000 hand-made draws, a grid of V = 32 values, weighted totals (``average=False``).

1  site side at ``--sites`` (200 000), 1 period x 1 visit: the fused call against the loop of V ``regional_totals(..., latent=False)``
   calls, one per grid value on the covariates with column 0 set to the value -- each opens a handle and uploads the data and the
   draws again.  The two return the same bytes, which is checked.
2  the fused site-side call alone at ``--grid-sites`` (10^6).
3  obs side, 1 period x 5 visits, against the host path: V calls of ``predict()`` on modified ``obs_covs`` and a NumPy reduction of
   ``prob_detection`` (n, J, T, N, 1) in float64.  The host path holds about 24 bytes per (draw, visit) -- the float32 array, the copy
   made while it is stacked, its float64 copy, the sums --: N is the largest multiple of 100 at which that is within 40 % of the memory
   available when the tool starts, and at most ``--max-obs-sites`` (so that the run stays within minutes).  The largest difference is
   printed as a fraction of the bound 2 (N - 1) 2^-53 sum |w v| (tests/curves_ref.py).
4  the fused obs-side call alone at ``--sites``, where the host path cannot run.

Everything runs in ONE process; every route gets a warm-up call at its full size first, then the routes of a comparison alternate
``--repeats`` times, a host clock around whole calls -- every call ends in a copy back to the host, so the device work is inside the
window.  One JSON line; ``--out`` also writes it to a file.  ``--only obs-grid`` runs the fourth part alone (to compare builds of the
obs kernel with another BL_RC_VALUE_BLOCK, BIOLITH_HIP_LIB=...).

    python tools/time_response_curves.py [--draws 4000] [--values 32] [--repeats 5] [--sites 200000] [--grid-sites 1000000] [--out F]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_response_curves.py --kernels   # one fused call a side after a warm-up"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K = 3
HOST_BYTES_PER_VISIT = 24


class _Posterior:
    def __init__(self, sites):
        self.sites = sites

    def get_samples(self):
        return self.sites


def _case(N, n, V, J):
    rng = np.random.default_rng(0)
    data = dict(site_covs=rng.normal(size=(N, K)).astype(np.float32), obs_covs=rng.normal(size=(N, 1, J, 1)).astype(np.float32))
    sites = dict(beta=rng.uniform(-1, 1, (n, 1, K + 1)).astype(np.float32), alpha=rng.uniform(-1, 1, (n, 1, 2)).astype(np.float32))
    return data, _Posterior(sites), np.linspace(-2.0, 2.0, V).astype(np.float32), rng.uniform(0.5, 2.0, N)


def _site_paths(N, n, V):
    from biolith_amd.models import occu
    from biolith_amd.utils import regional_totals, response_curves

    data, posterior, values, w = _case(N, n, V, 1)

    def fused():
        return response_curves(occu, posterior, **data, covariate=0, side="site", values=values, weights=w, average=False)["psi"]["draws"]

    def loop():
        columns = []
        for v in values:
            X = data["site_covs"].copy()
            X[:, 0] = v
            r = regional_totals(occu, posterior, site_covs=X, obs_covs=data["obs_covs"], weights=w, latent=False)
            columns.append(r["psi"]["draws"][:, 0])
        return np.stack(columns, axis=1)   # (n, V, 1)

    return fused, loop


def _obs_paths(N, n, V, J):
    from biolith_amd.models import occu
    from biolith_amd.utils import predict, response_curves

    data, posterior, values, w = _case(N, n, V, J)

    def fused():
        return response_curves(occu, posterior, **data, covariate=0, side="obs", values=values, weights=w, average=False)["prob_detection"]["draws"]

    def host():
        columns, bounds = [], []
        for v in values:
            W = data["obs_covs"].copy()
            W[..., 0] = v
            p = np.asarray(predict(occu, posterior, site_covs=data["site_covs"], obs_covs=W, num_samples=n)["prob_detection"])
            terms = w * p[..., 0].astype(np.float64).sum(axis=(1, 2))                      # (n, N)
            columns.append(terms.sum(axis=1))
            bounds.append(2.0 * (N - 1) * 2.0 ** -53 * np.abs(terms).sum(axis=1))
        return np.stack(columns, axis=1)[..., None], np.stack(bounds, axis=1)[..., None]

    return fused, host


def _available_bytes():
    with open("/proc/meminfo") as f:
        return next(int(line.split()[1]) for line in f if line.startswith("MemAvailable:")) * 1024


def _timed(call, name):
    t0 = time.perf_counter()
    call()
    wall = time.perf_counter() - t0
    print(f"{name}: {wall:.3f} s", file=sys.stderr, flush=True)
    return wall


def _alternate(routes, repeats):
    wall = {name: [] for name in routes}
    for _ in range(repeats):
        for name, call in routes.items():
            wall[name].append(_timed(call, name))
    return wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=4000)
    ap.add_argument("--values", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sites", type=int, default=200000)
    ap.add_argument("--grid-sites", type=int, default=1000000)
    ap.add_argument("--visits", type=int, default=5)
    ap.add_argument("--max-obs-sites", type=int, default=2000)
    ap.add_argument("--only", choices=["site", "grid", "obs", "obs-grid"], action="append", help="run this part alone (repeatable)")
    ap.add_argument("--out")
    ap.add_argument("--kernels", action="store_true", help="a warm-up call and one fused call a side, nothing else (for a kernel trace)")
    a = ap.parse_args()
    n, V, J = a.draws, a.values, a.visits
    parts = a.only or ["site", "grid", "obs", "obs-grid"]
    if a.kernels:
        for fused in (_site_paths(a.grid_sites, n, V)[0], _obs_paths(a.sites, n, V, J)[0]):
            fused()
            fused()
        return
    import biolith_amd._ffi as _ffi

    out = dict(shape=f"occu, {K} site covariates, {n} draws, {V} values, weighted totals", library=os.path.basename(_ffi.LIB_PATH))
    if "site" in parts:
        fused, loop = _site_paths(a.sites, n, V)
        want, got = loop(), fused()   # the warm-up call of each
        same = want.shape == got.shape and want.tobytes() == got.tobytes()
        del want, got
        wall = _alternate(dict(loop=loop, fused=fused), a.repeats)
        out["site"] = dict(sites=a.sites, visits="1 x 1", wall_s=wall, loop_wall_s_min=min(wall["loop"]), fused_wall_s_max=max(wall["fused"]),
                           fused_wall_s_min=min(wall["fused"]), loop_fastest_over_fused_slowest=min(wall["loop"]) / max(wall["fused"]),
                           fused_slowest_faster_than_loop_fastest=max(wall["fused"]) < min(wall["loop"]), same_bytes=same,
                           fused_site_draw_values_per_s=a.sites * n * V / min(wall["fused"]))
        del fused, loop
    if "grid" in parts:
        grid = _site_paths(a.grid_sites, n, V)[0]
        grid()
        wall = [_timed(grid, "grid") for _ in range(a.repeats)]
        out["grid"] = dict(sites=a.grid_sites, fused_wall_s=wall, fused_wall_s_min=min(wall), fused_wall_s_max=max(wall),
                           fused_site_draw_values_per_s=a.grid_sites * n * V / min(wall))
        del grid
    if "obs" in parts:
        available = _available_bytes()
        N = min(a.max_obs_sites, int(0.4 * available / (HOST_BYTES_PER_VISIT * n * J)) // 100 * 100)
        if N < 100:
            sys.exit(f"{available >> 20} MB available: the host path does not fit at 100 sites")
        fused, host = _obs_paths(N, n, V, J)
        (want, bound), got = host(), fused()   # the warm-up call of each
        error = float(np.max(np.abs(got - want) / bound))
        del want, got, bound
        wall = _alternate(dict(host=host, fused=fused), a.repeats)
        out["obs"] = dict(sites=N, visits=f"1 x {J}", sites_capped_by="--max-obs-sites" if N == a.max_obs_sites else "memory",
                          mem_available_mb=available >> 20, wall_s=wall, host_wall_s_min=min(wall["host"]), fused_wall_s_max=max(wall["fused"]),
                          fused_wall_s_min=min(wall["fused"]), host_fastest_over_fused_slowest=min(wall["host"]) / max(wall["fused"]),
                          error_as_fraction_of_bound=error, fused_visit_draw_values_per_s=N * J * n * V / min(wall["fused"]))
        del fused, host
    if "obs-grid" in parts:
        grid = _obs_paths(a.sites, n, V, J)[0]
        grid()
        wall = [_timed(grid, "obs-grid") for _ in range(a.repeats)]
        out["obs_grid"] = dict(sites=a.sites, visits=f"1 x {J}", fused_wall_s=wall, fused_wall_s_min=min(wall), fused_wall_s_max=max(wall),
                               fused_visit_draw_values_per_s=a.sites * J * n * V / min(wall))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
