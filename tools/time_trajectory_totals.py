"""Wall time of the trajectory totals of an occu_dyn posterior (utils.trajectory_totals) on a prediction grid, where the host path --
predict()'s (n, T, N) arrays -- cannot run: 3 site covariates, 10^6 cells, 4000 draws, T = 10 seasons, for 1 and for 100 regions, with
and without the realised path.

Every configuration runs in ONE process after a warm-up call of its own at the full size, the configurations alternating
(a, b, c, d, a, b, ...), a host clock around whole calls -- every call ends in a copy back to the host, so the device work is inside the
window; the median, the smallest and the largest of ``--repeats`` calls are reported.  A call opens its handle (the site covariates go
up) and lays the slots out; ``parts`` times the engine's method alone on an open handle for single outputs, one region -- the
equilibrium alone is the rates and one block of rows reduced a draw, the occupancy alone T blocks and the recursion on top, and so on --,
and for all outputs in 100 regions, which leaves out the wrapper's host side (the labels' ``np.unique``, NumPy's mean, sd and quantiles
of nine (n, T, G) arrays).  One JSON line; ``--out`` also writes it to a file.

    python tools/time_trajectory_totals.py [--sites 1000000] [--draws 4000] [--periods 10] [--repeats 5] [--out F]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_trajectory_totals.py --kernels [--regions 100]   # one call, all outputs, after a warm-up"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K = 3
PARTS = (("equilibrium",), ("occupancy",), ("occupancy", "colonised", "extinct", "equilibrium"), ("z",), ("z", "z_colonised", "z_extinct"),
         ("occupancy", "colonised", "extinct", "equilibrium", "z", "z_colonised", "z_extinct"))


class _Posterior:
    def __init__(self, sites):
        self.sites = sites

    def get_samples(self):
        return self.sites


def _case(N, n):
    rng = np.random.default_rng(0)
    sites = {k: rng.uniform(-1, 1, (n, 1, K + 1)).astype(np.float32) for k in ("beta", "beta_col", "beta_ext")}
    sites["alpha"] = rng.uniform(-1, 1, (n, 1, 2)).astype(np.float32)
    return rng.normal(size=(N, K)).astype(np.float32), _Posterior(sites), rng.uniform(0.5, 2.0, N)


def _wall(call):
    t0 = time.perf_counter()
    call()
    return time.perf_counter() - t0


def _summary(wall):
    return dict(wall_s=wall, median_s=statistics.median(wall), min_s=min(wall), max_s=max(wall))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=1000000)
    ap.add_argument("--draws", type=int, default=4000)
    ap.add_argument("--periods", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--kernels", action="store_true", help="a warm-up call and one call (--regions, all outputs), nothing else (for a kernel trace)")
    ap.add_argument("--regions", type=int, default=100, choices=(1, 100), help="the regions of the --kernels call")
    a = ap.parse_args()
    from biolith_amd.engine import OccuDataset
    from biolith_amd.models import occu_dyn
    from biolith_amd.utils import trajectory_totals

    N, n, T = a.sites, a.draws, a.periods
    X, posterior, w = _case(N, n)
    labels = {1: None, 100: np.random.default_rng(1).integers(0, 100, N)}
    call = lambda G, latent: trajectory_totals(occu_dyn, posterior, site_covs=X, n_periods=T, regions=labels[G], weights=w, latent=latent,
                                               random_seed=1)
    if a.kernels:
        call(a.regions, True)
        call(a.regions, True)
        return
    configs = [(G, latent) for G in (1, 100) for latent in (False, True)]
    for c in configs:   # the warm-up call of each
        print(f"warm-up regions={c[0]} latent={c[1]}: {_wall(lambda: call(*c)):.3f} s", file=sys.stderr, flush=True)
    wall = {c: [] for c in configs}
    for _ in range(a.repeats):
        for c in configs:
            wall[c].append(_wall(lambda: call(*c)))
            print(f"regions={c[0]} latent={c[1]}: {wall[c][-1]:.3f} s", file=sys.stderr, flush=True)
    out = dict(shape=f"occu_dyn, {K} site covariates, {N} sites, {n} draws, {T} periods", sites=N, draws=n, periods=T,
               calls={f"regions={G},latent={latent}": dict(_summary(wall[(G, latent)]), site_draws_per_s=N * n / statistics.median(wall[(G, latent)]))
                      for G, latent in configs})
    # the engine's method alone on an open handle, one region, output by output
    s = posterior.sites
    ds = OccuDataset(X, np.zeros((N, 1, 1, 1), dtype=np.float32), np.full((1, N, 1, 1), np.nan, dtype=np.float32), model="occu_dyn")
    draws = np.ascontiguousarray(np.concatenate([s[k][:, 0] for k in ("beta", "beta_col", "beta_ext", "alpha")], axis=1))
    region = np.zeros(N, dtype=np.int32)
    part = lambda names: ds.trajectory_totals(draws, region, 1, T, weight=w, seed=1, outputs=names)
    for names in PARTS:
        part(names)
    walls = {names: [] for names in PARTS}
    for _ in range(a.repeats):
        for names in PARTS:
            walls[names].append(_wall(lambda: part(names)))
    every = lambda: ds.trajectory_totals(draws, labels[100], 100, T, weight=w, seed=1)   # all outputs, 100 regions: the call without its host side
    every()
    wall_every = [_wall(every) for _ in range(a.repeats)]
    ds.close()
    rows = dict(occupancy=T, colonised=T - 1, extinct=T - 1, equilibrium=1, z=T, z_colonised=T - 1, z_extinct=T - 1)
    out["parts"] = {"+".join(names): dict(_summary(walls[names]), reductions_per_draw=sum(rows[k] for k in names)) for names in PARTS}
    out["engine_all_outputs_100_regions"] = _summary(wall_every)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
