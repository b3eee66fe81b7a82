"""Probes at the edges of the workgroups' slices, through bl_logp_grad.

A site covariate that is 1 at one chosen site and 0 everywhere else (or an observation covariate that is 1 at one (site, period, visit))
has a coefficient whose gradient is that one site's (visit's) term plus its prior.  A slice that starts one site late, a half-filled
last pair that is dropped, a last visit that is never read or a site on the wrong side of occu_rn's detected / closed-form split then
moves that coordinate by its whole size, however small the site is next to the rest of the data.  So each probe coordinate is compared
with the float64 oracle relative to its OWN magnitude:  |dG_k| <= r (|G_k - prior_k| + |prior_k|),  not relative to max|G|.

The positions come from the geometry a one-chain launch reports (wgs_per_chain k, nloc = ceil(N / k) sites per workgroup): the
geometry bl_logp_grad picks (choose_geometry for one chain)."""
import numpy as np
import pytest

import oracle
from biolith_amd.engine import OccuDataset
from conftest import load_golden, quiet_simulate
from test_gpu_rn import _rn_data

pytestmark = pytest.mark.gpu

# r per family; the measured maximum of |dG_k| / (|G_k - prior_k| + |prior_k|) over the probes (MI355X) beside it
PROBE_RTOL = {
    "occu": 2e-6,   # measured 4.8e-7
    "fp": 2e-6,     # measured 6.3e-7
    "rn": 2e-6,     # measured 6.9e-7
    "cop": 1e-6,    # measured 6.9e-8
    "nmix": 1e-6,   # measured 1.1e-7
    "re": 1e-6,     # measured 1.2e-7
}
MAX_PROBES = 8      # indicator columns per side in one dataset (16 covariates at most, with the data's own)


def _with_indicators(X, Wc, sites, visits):
    """X and W with one indicator column per probe appended: site s (X) / visit (n, t, j) (W)."""
    N, T, J, _ = Wc.shape
    Xs = np.zeros((N, len(sites)), np.float32)
    for c, s in enumerate(sites):
        Xs[s, c] = 1.0
    Wo = np.zeros((N, T, J, len(visits)), np.float32)
    for c, (n, t, j) in enumerate(visits):
        Wo[n, t, j, c] = 1.0
    return np.concatenate([X, Xs], 1), np.concatenate([Wc, Wo], 3)


def _slice_edges(N, k):
    nloc = -(-N // k)
    out = []
    for w in range(k):
        a, b = w * nloc, min(N, (w + 1) * nloc) - 1
        if a <= b:
            out += [a, b]
    return sorted(set(out + [N - 1]))


def _geometry(X, Wc, Y, kw, n_site_probes, n_visit_probes):
    """(k, nloc) of a one-chain launch on data of the probes' shape (the geometry depends on the shape alone)."""
    Xp, Wp = _with_indicators(X, Wc, [0] * n_site_probes, [(0, 0, 0)] * n_visit_probes)
    ds = OccuDataset(Xp, Wp, Y, **kw)
    r = ds.nuts(num_warmup=0, num_samples=1, num_chains=1, seed=0)
    k = r.wgs_per_chain
    ds.close()
    return k, -(-X.shape[0] // k)


def _probe(X, Wc, Y, kw, sites, visits, family, seed=0):
    """K1 at indicator covariates of `sites` and `visits`; returns the worst per-coordinate ratio to the bound."""
    Xp, Wp = _with_indicators(X, Wc, sites, visits)
    od = oracle.OracleData(Xp, Wp, Y, **kw)
    ds = OccuDataset(Xp, Wp, Y, **kw)
    Ks0, Ko0 = X.shape[1], Wc.shape[3]
    ib = [1 + Ks0 + c for c in range(len(sites))]                          # beta: intercept, the data's, the probes'
    ia = [1 + Xp.shape[1] + 1 + Ko0 + c for c in range(len(visits))]       # alpha behind beta
    rng = np.random.default_rng(seed)
    th = rng.uniform(-0.8, 0.8, size=(2, od.D))
    th[:, ib + ia] = rng.uniform(-1.5, 1.5, size=(2, len(ib) + len(ia)))
    th = th.astype(np.float32).astype(np.float64)
    Uo, Go = od.potential_grad(th)
    Ug, Gg = ds.logp_grad(th)
    ds.close()
    assert np.all(np.isfinite(Ug)) and np.all(np.isfinite(Gg))
    idx = ib + ia
    prior = th[:, idx]                      # Normal(0, 1) on every coefficient: dU/dtheta_k of the prior = theta_k
    dG = np.abs(Gg[:, idx] - Go[:, idx])
    scale = np.abs(Go[:, idx] - prior) + np.abs(prior)
    # the site (visit) term must be there at all: an indicator of a site that reaches the likelihood has a non-zero term
    assert np.all(np.abs(Go[:, idx] - prior) > 0), (sites, visits)
    ratio = dG / (PROBE_RTOL[family] * scale)
    b, c = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    where = sites[c] if c < len(sites) else visits[c - len(sites)]
    measured = float(np.max(dG / scale))
    print(f"\nPROBE {family} sites={sites} visits={visits} max|dG|/scale={measured:.3g}")
    assert ratio[b, c] <= 1.0, (f"{family}: probe at {where} (theta row {b}): kernel {Gg[b, idx[c]]!r} oracle {Go[b, idx[c]]!r} "
                                f"prior {prior[b, c]!r}: {dG[b, c] / scale[b, c]:.3g} of its own size, bound {PROBE_RTOL[family]:g}")
    return measured


def _run_probes(X, Wc, Y, kw, family, extra_sites=(), min_k=1):
    """Every slice's first and last site, the last site, `extra_sites`; the last visit of the last period of the last site and of
    the first slice's last site, and the first visit of the first site."""
    N, T, J, _ = Wc.shape
    ks, kv = min(MAX_PROBES, 16 - X.shape[1]), min(3, 16 - Wc.shape[3])
    k, nloc = _geometry(X, Wc, Y, kw, ks, kv)
    assert k >= min_k, k
    sites = sorted(set(_slice_edges(N, k)) | set(extra_sites))
    visits = list(dict.fromkeys([(N - 1, T - 1, J - 1), (min(nloc, N) - 1, T - 1, J - 1), (0, 0, 0)]))[:kv]
    Y, Wc = np.array(Y, dtype=np.float32), np.array(Wc, dtype=np.float32)
    for n, t, j in visits:             # a probed visit is observed (a missing one has no term to probe)
        Y[0, n, t, j] = np.nan_to_num(Y[0, n, t, j])
        Wc[n, t, j] = np.nan_to_num(Wc[n, t, j])
    worst = 0.0
    for i in range(0, len(sites), ks):
        worst = max(worst, _probe(X, Wc, Y, kw, sites[i:i + ks], visits if i == 0 else [], family, seed=i))
    print(f"PROBES {family} N={N} k={k} nloc={nloc} sites={len(sites)} worst={worst:.3g}")
    return k


def test_occu_slice_edges():
    """Plain occu, odd N (the last pair half filled), three periods: every slice's edges and the last visit of the last period."""
    d, _, _ = quiet_simulate(n_sites=4001, n_periods=3, n_site_covs=2, n_obs_covs=1, deployment_days_per_site=35, session_duration=7, random_seed=8)
    _run_probes(d["site_covs"], d["obs_covs"], d["obs"], {}, "occu", min_k=2)


def test_occu_fp_slice_edges():
    d, _, _ = quiet_simulate(n_sites=2999, n_site_covs=2, n_obs_covs=1, deployment_days_per_site=35, session_duration=7, prob_fp_constant=0.1,
                             random_seed=4)
    _run_probes(d["site_covs"], d["obs_covs"], d["obs"], dict(model="occu_fp", fp_mode="constant"), "fp", min_k=2)


def test_occu_rn_slice_edges_and_the_split():
    """occu_rn at config 4's proportions (the split is on): slice edges, and in the first and last slices the first and last site with a
    detection and without one -- the sites on either side of the detected / closed-form boundary once a workgroup has sorted them."""
    X, Wc, Y = _rn_data(np.random.default_rng(21), 5001, 10, 0.34)
    kw = dict(model="occu_rn")
    k, nloc = _geometry(X, Wc, Y, kw, MAX_PROBES, 3)
    N = X.shape[0]
    det = np.nan_to_num(Y[0]).reshape(N, -1).sum(1) > 0
    extra = []
    for w in (0, k - 1):
        a, b = w * nloc, min(N, (w + 1) * nloc)
        for flag in (True, False):
            s = np.nonzero(det[a:b] == flag)[0]
            if s.size:
                extra += [a + int(s[0]), a + int(s[-1])]
    assert _run_probes(X, Wc, Y, kw, "rn", extra_sites=extra, min_k=2) == k


def test_occu_cop_slice_edges():
    g = load_golden("cop_default")
    _run_probes(g["site_covs"], g["obs_covs"], g["obs"], dict(model="occu_cop", fp_mode=None, session_duration=g["session_duration"]), "cop")


def test_nmixture_slice_edges():
    g = load_golden("nmix_ref_test")
    _run_probes(g["site_covs"], g["obs_covs"], g["obs"], dict(model="nmixture"), "nmix")


def test_random_effects_slice_edges():
    """The random-effects path (re_logp_grad) at 2 001 sites, site effects."""
    d, _, _ = quiet_simulate(n_sites=2001, n_site_covs=2, n_obs_covs=1, deployment_days_per_site=35, session_duration=7,
                             site_random_effects=True, random_seed=5)
    _run_probes(d["site_covs"], d["obs_covs"], d["obs"], dict(model="occu_re", site_random_effects=True), "re", min_k=2)
