"""Wall time of species richness across the species of an occu posterior (utils.species_richness): 3 site covariates, 4000 draws,
S = 8 species unless told otherwise.  Three measurements, one per ``--mode``, each in ONE process after a warm-up call of its own at the
full size, a host clock around whole calls -- every call ends in a copy back to the host, so the device work is inside the window;
the median, the smallest and the largest of ``--repeats`` calls are reported:

  host   the host path at a size the host holds (2000 sites): predict()'s psi of the S species followed by the NumPy recursion, the
         site means and the one region's area, against the fused call
  loop   a loop of S regional_totals(..., latent=False) calls, one single-species posterior each, one region (200 000 sites) -- it
         returns only what adds up to ``richness`` --, against the fused call; the two alternate
  grid   the engine's method on an open handle at 10^6 sites, one region: the area alone, the site outputs alone, both; S = 8 and 32

One JSON line; ``--out`` also writes it to a file.

    python tools/time_species_richness.py --mode host|loop|grid [--sites N] [--draws 4000] [--species 8] [--repeats 5] [--out F]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_species_richness.py --mode loop --kernels fused|loop   # one call after a warm-up"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K = 3
SITES = dict(host=2000, loop=200000, grid=1000000)


class _Posterior:
    def __init__(self, sites):
        self.sites = sites

    def get_samples(self):
        return self.sites


def _case(N, n, S):
    rng = np.random.default_rng(0)
    sites = dict(beta=rng.uniform(-1, 1, (n, S, K + 1)).astype(np.float32), alpha=rng.uniform(-1, 1, (n, S, 2)).astype(np.float32))
    data = dict(site_covs=rng.normal(size=(N, K)).astype(np.float32), obs_covs=np.zeros((N, 1, 1, 1), dtype=np.float32))
    return data, _Posterior(sites), rng.uniform(0.5, 2.0, N)


def _wall(call):
    t0 = time.perf_counter()
    call()
    return time.perf_counter() - t0


def _summary(wall):
    return dict(wall_s=wall, median_s=statistics.median(wall), min_s=min(wall), max_s=max(wall))


def _alternate(calls, repeats):
    """{name: call} -> {name: summary}: a warm-up of each, then the calls alternating."""
    for name, call in calls.items():
        print(f"warm-up {name}: {_wall(call):.3f} s", file=sys.stderr, flush=True)
    wall = {name: [] for name in calls}
    for _ in range(repeats):
        for name, call in calls.items():
            wall[name].append(_wall(call))
            print(f"{name}: {wall[name][-1]:.3f} s", file=sys.stderr, flush=True)
    return {name: _summary(w) for name, w in wall.items()}


def _host_path(occu, predict, posterior, data, w, n):
    """predict()'s psi, then the recursion over the species, the site means and one region's area in NumPy."""
    psi32 = np.asarray(predict(occu, posterior, **data, num_samples=n, random_seed=0)["psi"])[:, 0]   # (n, N, S)
    S = psi32.shape[-1]
    pmf, area = np.zeros(psi32.shape[1:-1] + (S + 1,)), []
    for n0 in range(0, n, 500):   # (500 draws at a time: the float64 arrays of all of them are several GB)
        psi = psi32[n0:n0 + 500].astype(np.float64)
        pi = np.zeros(psi.shape[:-1] + (S + 1,))
        pi[..., 0] = 1.0
        for s in range(S):
            p = psi[..., s, None]
            shifted = np.concatenate([np.zeros(pi.shape[:-1] + (1,)), pi[..., :-1]], axis=-1)
            pi = pi * (1.0 - p) + shifted * p
        pmf += pi.sum(axis=0)
        area.append(np.einsum("i,nir->nr", w, pi))
    E = psi32.sum(axis=-1, dtype=np.float64)
    return pmf / n, E.mean(axis=0), E.std(axis=0, ddof=1), np.concatenate(area)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=tuple(SITES), required=True)
    ap.add_argument("--sites", type=int)
    ap.add_argument("--draws", type=int, default=4000)
    ap.add_argument("--species", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--kernels", choices=("fused", "loop"), help="mode loop: a warm-up call and one call of this side, nothing else (for a kernel trace)")
    a = ap.parse_args()
    from biolith_amd.engine import OccuDataset
    from biolith_amd.models import occu
    from biolith_amd.utils import predict, regional_totals, species_richness

    N, n, S = a.sites or SITES[a.mode], a.draws, a.species
    out = dict(mode=a.mode, sites=N, draws=n, species=S, shape=f"occu, {K} site covariates, {N} sites, {n} draws")
    data, posterior, w = _case(N, n, S)
    if a.mode == "host":
        out["calls"] = _alternate({"predict_and_numpy": lambda: _host_path(occu, predict, posterior, data, w, n),
                                   "fused": lambda: species_richness(occu, posterior, **data, weights=w)}, a.repeats)
    elif a.mode == "loop":
        singles = [_Posterior({k: np.ascontiguousarray(v[:, s:s + 1]) for k, v in posterior.sites.items()}) for s in range(S)]
        calls = {"loop_of_regional_totals": lambda: [regional_totals(occu, one, **data, weights=w, latent=False) for one in singles],
                 "fused": lambda: species_richness(occu, posterior, **data, weights=w, per_site=False),
                 "fused_with_site": lambda: species_richness(occu, posterior, **data, weights=w)}
        if a.kernels:
            call = calls["fused" if a.kernels == "fused" else "loop_of_regional_totals"]
            call()
            call()
            return
        out["calls"] = _alternate(calls, a.repeats)
    else:
        out["calls"] = {}
        for S_ in (8, 32):
            data, posterior, w = _case(N, n, S_)
            ds = OccuDataset(data["site_covs"], data["obs_covs"], np.full((1, N, 1, 1), np.nan, dtype=np.float32))
            s = posterior.sites
            draws = np.ascontiguousarray(np.concatenate([s["beta"], s["alpha"]], axis=2))   # (n, S, D): [beta | alpha] a species
            assert draws.shape[2] == ds.D
            region = np.zeros(N, dtype=np.int32)
            calls = {f"S={S_},area": lambda: ds.species_richness(draws, region, 1, weight=w, site=False),
                     f"S={S_},site": lambda: ds.species_richness(draws, area=False),
                     f"S={S_},both": lambda: ds.species_richness(draws, region, 1, weight=w)}
            out["calls"].update(_alternate(calls, a.repeats))
            ds.close()
    for name, c in out["calls"].items():
        c["site_draws_per_s"] = N * n / c["median_s"]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
