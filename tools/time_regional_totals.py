"""Wall time of the regional totals, fused (utils.regional_totals) against the host path (predict(), then per region
``(w[idx] * preds[site][..., idx]).sum`` per draw, in float64) on the same inputs: occu, 3 site covariates, 1 period x 1 visit, 4000
draws, 32 regions, both totals (psi and z).

The host path holds predict()'s (n, T, N) arrays -- psi float32, z int32 and the copies made while they are stacked --, about 32 bytes per
(draw, site): N is the largest multiple of 1000 at which that is within 40 % of the memory available when the tool starts, and at most
``--max-sites`` (so that the run stays within minutes).  Both paths run in ONE process, after a warm-up call of each at the full size,
alternating (host, fused, host, fused, ...), a host clock around whole calls -- every call ends in a copy back to the host, so the device
work is inside the window.  Then the fused call alone at ``--grid-sites`` (10^6), where the host path cannot run.  The largest error of
the fused result against the host path's is printed as a fraction of the bound of tests/totals_ref.py.  One JSON line; ``--out`` also
writes it to a file.

    python tools/time_regional_totals.py [--draws 4000] [--regions 32] [--repeats 5] [--max-sites 200000] [--grid-sites 1000000] [--out F]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_regional_totals.py --kernels     # one fused grid call after a warm-up"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K = 3
HOST_BYTES_PER_CELL = 32


class _Posterior:
    def __init__(self, sites):
        self.sites = sites

    def get_samples(self):
        return self.sites


def _case(N, n, G):
    rng = np.random.default_rng(0)
    data = dict(site_covs=rng.normal(size=(N, K)).astype(np.float32), obs_covs=rng.normal(size=(N, 1, 1, 1)).astype(np.float32))
    sites = dict(beta=rng.uniform(-1, 1, (n, 1, K + 1)).astype(np.float32), alpha=rng.uniform(-1, 1, (n, 1, 2)).astype(np.float32))
    return data, _Posterior(sites), rng.integers(0, G, N), rng.uniform(0.5, 2.0, N)


def _paths(N, n, G):
    from biolith_amd.models import occu
    from biolith_amd.utils import predict, regional_totals

    data, posterior, regions, w = _case(N, n, G)
    sites = [np.flatnonzero(regions == g) for g in range(G)]

    def fused():
        r = regional_totals(occu, posterior, **data, regions=regions, weights=w, random_seed=1)
        return r["psi"]["draws"], r["z"]["draws"]

    def host():
        preds = predict(occu, posterior, **data, num_samples=n, random_seed=1)
        psi, z = np.asarray(preds["psi"])[:, 0, :, 0], np.asarray(preds["z"])[:, :, :, 0]
        first = np.stack([np.sum(w[idx] * psi[:, idx].astype(np.float64), axis=-1) for idx in sites], axis=-1)
        second = np.stack([np.sum(w[idx] * z[:, :, idx].astype(np.float64), axis=-1) for idx in sites], axis=-1)
        return first[..., None], second[..., None]

    def bound():   # 2 (N_g - 1) 2^-53 sum |w v|, v <= 1
        return np.array([2.0 * (len(idx) - 1) * 2.0 ** -53 * np.abs(w[idx]).sum() for idx in sites])

    return fused, host, bound


def _available_bytes():
    with open("/proc/meminfo") as f:
        return next(int(line.split()[1]) for line in f if line.startswith("MemAvailable:")) * 1024


def _timed(call, repeats):
    wall = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        wall.append(time.perf_counter() - t0)
        print(f"{getattr(call, '__name__', 'call')}: {wall[-1]:.3f} s", file=sys.stderr, flush=True)
    return wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=4000)
    ap.add_argument("--regions", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-sites", type=int, default=200000)
    ap.add_argument("--grid-sites", type=int, default=1000000)
    ap.add_argument("--out")
    ap.add_argument("--kernels", action="store_true", help="a warm-up call and one fused call at --grid-sites, nothing else (for a kernel trace)")
    a = ap.parse_args()
    n, G = a.draws, a.regions
    if a.kernels:
        fused = _paths(a.grid_sites, n, G)[0]
        fused()
        fused()
        return
    available = _available_bytes()
    N = min(a.max_sites, int(0.4 * available / (HOST_BYTES_PER_CELL * n)) // 1000 * 1000)
    if N < 1000:
        sys.exit(f"{available >> 20} MB available: the host path does not fit at 1000 sites")
    fused, host, bound = _paths(N, n, G)
    want, got = host(), fused()   # the warm-up call of each
    b = bound()
    error = [float(np.max(np.abs(g - w_) / b[:, None])) for g, w_ in zip(got, want)]
    del want, got
    wall = dict(host=[], fused=[])
    for _ in range(a.repeats):
        wall["host"] += _timed(host, 1)
        wall["fused"] += _timed(fused, 1)
    out = dict(shape=f"occu, {K} site covariates, 1 period x 1 visit, {n} draws, {G} regions, psi and z",
               sites=N, sites_capped_by="--max-sites" if N == a.max_sites else "memory", mem_available_mb=available >> 20, wall_s=wall,
               host_wall_s_min=min(wall["host"]), fused_wall_s_max=max(wall["fused"]), fused_wall_s_min=min(wall["fused"]),
               fused_slowest_faster_than_host_fastest=max(wall["fused"]) < min(wall["host"]),
               fused_site_draws_per_s=N * n / min(wall["fused"]), host_site_draws_per_s=N * n / min(wall["host"]),
               error_as_fraction_of_bound=dict(psi=error[0], z=error[1]))
    del fused, host
    grid = _paths(a.grid_sites, n, G)[0]
    grid()
    wall_grid = _timed(grid, a.repeats)
    out["grid"] = dict(sites=a.grid_sites, fused_wall_s=wall_grid, fused_wall_s_min=min(wall_grid), fused_wall_s_max=max(wall_grid),
                       fused_site_draws_per_s=a.grid_sites * n / min(wall_grid))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
