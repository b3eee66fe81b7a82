"""Wall time of the residuals' Moran's I (utils.residual_moran): occu, 3 site covariates, 1 visit covariate, T = 1, J = 3, 4000 draws,
a row-standardised graph of the k = 8 nearest neighbours of uniform random coordinates, unless told otherwise.  Two measurements, one
per ``--mode``, each in ONE process after a warm-up call of its own at the full size, a host clock around whole calls -- every call
ends in a copy back to the host, so the device work is inside the window; the median, the smallest and the largest of ``--repeats``
calls are reported:

  host   at a size the host holds (2000 sites): conditional_occupancy + predict + evaluation.residuals and a sparse Moran's I per
         draw in NumPy / SciPy, against the fused wrapper call on the same graph; the two alternate
  grid   the engine's method on an open handle (10^5 sites; ``--sites`` for 10^6): Moran's I alone, the site outputs alone, both

One JSON line; ``--out`` also writes it to a file.

    python tools/time_residual_moran.py --mode host|grid [--sites N] [--draws 4000] [--repeats 5] [--out F]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_residual_moran.py --mode grid --kernels   # one call after a warm-up"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K, J, NEIGHBOURS = 3, 3, 8
SITES = dict(host=2000, grid=100000)


class _Posterior:
    def __init__(self, sites):
        self.sites = sites

    def get_samples(self):
        return self.sites


def _case(N, n):
    rng = np.random.default_rng(0)
    sites = dict(beta=rng.uniform(-1, 1, (n, 1, K + 1)).astype(np.float32), alpha=rng.uniform(-1, 1, (n, 1, 2)).astype(np.float32))
    data = dict(site_covs=rng.normal(size=(N, K)).astype(np.float32), obs_covs=rng.normal(size=(N, 1, J, 1)).astype(np.float32),
                obs=(rng.random((1, N, 1, J)) < 0.3).astype(np.float32))
    return data, _Posterior(sites), rng.random((N, 2))


def _wall(call):
    t0 = time.perf_counter()
    call()
    return time.perf_counter() - t0


def _alternate(calls, repeats):
    """{name: call} -> {name: summary}: a warm-up of each, then the calls alternating."""
    for name, call in calls.items():
        print(f"warm-up {name}: {_wall(call):.3f} s", file=sys.stderr, flush=True)
    wall = {name: [] for name in calls}
    for _ in range(repeats):
        for name, call in calls.items():
            wall[name].append(_wall(call))
            print(f"{name}: {wall[name][-1]:.3f} s", file=sys.stderr, flush=True)
    return {name: dict(wall_s=w, median_s=statistics.median(w), min_s=min(w), max_s=max(w)) for name, w in wall.items()}


def _sparse_moran(v, A):
    """Moran's I of every row of the masked fields ``v`` (n, N), NaN = outside, over the sparse matrix ``A``: a product per draw."""
    I = np.full(v.shape[0], np.nan)
    for k in range(v.shape[0]):
        m = np.isfinite(v[k])
        if m.sum() < 2:
            continue
        c = np.where(m, v[k] - v[k][m].mean(), 0.0)
        mf = m.astype(np.float64)
        W, den = mf @ (A @ mf), c @ c
        if W != 0.0 and den > 0.0:
            I[k] = m.sum() / W * (c @ (A @ c)) / den
    return I


def _host_path(occu, posterior, data, graph, n):
    """conditional_occupancy + predict + residuals, then per draw a sparse Moran's I of the four fields (T = 1, one species)."""
    import scipy.sparse as sp

    from biolith_amd.evaluation.predictive_checks import residuals
    from biolith_amd.utils import conditional_occupancy, predict

    N = data["site_covs"].shape[0]
    A = sp.csr_matrix((graph[2], graph[1], graph[0]), shape=(N, N))
    lat = conditional_occupancy(occu, posterior, **data, random_seed=0)
    preds = predict(occu, posterior, data["site_covs"], data["obs_covs"], num_samples=n, random_seed=1)
    both = {k: np.asarray(preds[k]) for k in ("psi", "prob_detection", "z", "y")}
    o_obs, d_obs = residuals({**both, "z": np.asarray(lat["z"])}, data["obs"])                # (n, T, N, S), (n, S, N, T, J)
    o_rep = both["z"] - both["psi"].astype(np.float64)
    d_rep = np.where(both["z"][:, None] == 1, both["y"] - both["prob_detection"].astype(np.float64), np.nan).transpose(0, 4, 3, 2, 1)
    site_level = lambda d: np.nanmean(d[:, 0, :, 0, :], axis=-1)                                # (n, N): over the visits
    return [_sparse_moran(v, A) for v in (o_obs[:, 0, :, 0], o_rep[:, 0, :, 0], site_level(d_obs), site_level(d_rep))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=tuple(SITES), required=True)
    ap.add_argument("--sites", type=int)
    ap.add_argument("--draws", type=int, default=4000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--kernels", action="store_true", help="mode grid: a warm-up call and one call with every output, nothing else (for a kernel trace)")
    a = ap.parse_args()
    import warnings

    from biolith_amd.engine import OccuDataset
    from biolith_amd.models import occu
    from biolith_amd.utils import neighbour_graph, residual_moran

    N, n = a.sites or SITES[a.mode], a.draws
    out = dict(mode=a.mode, sites=N, draws=n, k=NEIGHBOURS, shape=f"occu, {K} site covariates, J = {J}, {N} sites, {n} draws, kNN k = {NEIGHBOURS}")
    data, posterior, xy = _case(N, n)
    t0 = time.perf_counter()
    graph = neighbour_graph(xy, k=NEIGHBOURS)
    out["graph_s"] = time.perf_counter() - t0
    if a.mode == "host":
        warnings.simplefilter("ignore")   # (nanmean of a site no draw has occupied)
        out["calls"] = _alternate({"host_path": lambda: _host_path(occu, posterior, data, graph, n),
                                   "fused": lambda: residual_moran(occu, posterior, **data, neighbours=graph)}, a.repeats)
    else:
        ds = OccuDataset(data["site_covs"], data["obs_covs"], data["obs"])
        s = posterior.sites
        draws = np.ascontiguousarray(np.concatenate([s["beta"][:, 0], s["alpha"][:, 0]], axis=1))   # (n, D): [beta | alpha]
        assert draws.shape[1] == ds.D
        calls = {"moran": lambda: ds.residual_moran(draws, graph, site=False), "site": lambda: ds.residual_moran(draws, None, moran=False),
                 "both": lambda: ds.residual_moran(draws, graph)}
        if a.kernels:
            calls["both"]()
            calls["both"]()
            return
        out["calls"] = _alternate(calls, a.repeats)
        ds.close()
    for c in out["calls"].values():
        c["site_draws_per_s"] = N * n / c["median_s"]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
