"""Conditional abundance without a GPU: the float64 restatement (tests/abundance_ref.py) pinned to the densities the project already
trusts (oracle.literal_log_joint_rn / _nmix, the committed fixtures of the reference's own models), its structure, the host-side
criteria (finite_sample_abundance, waic_marginal on such a result) and the Python refusals."""
import contextlib
import io

import numpy as np
import pytest
from scipy import stats
from scipy.special import gammaln, logsumexp

import abundance_ref as A
import oracle
import reference_logjoint as R
from biolith_amd import _ffi, models
from biolith_amd.evaluation import finite_sample_abundance, lppd_marginal, waic_marginal
from biolith_amd.models import simulate_nmixture, simulate_rn
from biolith_amd.utils import conditional_abundance
from latent_ref import occu_theta_layout

TINY = float(np.finfo(np.float32).tiny)


log_prior = A.log_prior


def _sim(fn, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        data, truth = fn(**kw)
    return np.asarray(data["site_covs"]), np.asarray(data["obs_covs"]), np.asarray(data["obs"])[0]


def _theta(rng, D, n_coef, scale=0.8):
    th = rng.uniform(-scale, scale, size=D)
    th[n_coef:] *= 0.5    # the rate, the log sds and the effects
    return th


RN_CASES = {
    "default": (dict(), dict()),
    "missing": (dict(simulate_missing=True, random_seed=1), dict()),
    "two_periods": (dict(n_periods=2, n_sites=60, deployment_days_per_site=70, simulate_missing=True, random_seed=2), dict()),
    "fp_constant": (dict(n_sites=60, deployment_days_per_site=70, random_seed=3), dict(fp=True)),
    "site_effects": (dict(n_sites=50, n_periods=2, deployment_days_per_site=49, random_seed=4), dict(site_re=True)),
    "obs_effects": (dict(n_sites=50, deployment_days_per_site=49, simulate_missing=True, random_seed=5), dict(obs_re=True, fp=True)),
}
NMIX_CASES = {
    "default": (dict(), dict()),
    "missing": (dict(simulate_missing=True, random_seed=1), dict()),
    "two_periods": (dict(n_periods=2, n_sites=60, deployment_days_per_site=70, simulate_missing=True, random_seed=2), dict()),
    "site_effects": (dict(n_sites=50, n_periods=2, deployment_days_per_site=49, random_seed=4), dict(site_re=True)),
    "obs_effects": (dict(n_sites=50, deployment_days_per_site=49, simulate_missing=True, random_seed=5), dict(obs_re=True, site_re=True)),
}


@pytest.mark.parametrize("case", sorted(RN_CASES))
def test_rn_cells_sum_to_the_literal_log_joint(case):
    sim, opt = RN_CASES[case]
    X, W, Y = _sim(simulate_rn, **sim)
    N, T, J, Ko = W.shape
    fp, site, obs = opt.get("fp", False), opt.get("site_re", False), opt.get("obs_re", False)
    D = occu_theta_layout(N, T, J, X.shape[1], Ko, fp, site, obs)["D"]
    rng = np.random.default_rng(len(case))
    for K in (100, 20):
        th = _theta(rng, D, X.shape[1] + Ko + 2)
        c = A.rn_cells(X, W, Y, th, K, fp=fp, site_re=site, obs_re=obs)
        lj = oracle.literal_log_joint_rn(th, X, W, Y, max_abundance=K, site_random_effects=site, obs_random_effects=obs, false_positives_constant=fp)
        want = lj - log_prior(th, N, T, J, X.shape[1], Ko, fp, site, obs)
        assert abs(c["l"].sum() - want) <= 1e-10 * abs(want), (case, K, c["l"].sum(), want)
        assert c["l"].shape == (T, N) and c["pmf"].shape == (T, N, K + 1)
        assert np.max(np.abs(c["pmf"].sum(-1) - 1.0)) <= 1e-12


@pytest.mark.parametrize("case", sorted(NMIX_CASES))
def test_nmix_cells_sum_to_the_literal_log_joint(case):
    sim, opt = NMIX_CASES[case]
    X, W, Y = _sim(simulate_nmixture, **sim)
    N, T, J, Ko = W.shape
    site, obs = opt.get("site_re", False), opt.get("obs_re", False)
    D = occu_theta_layout(N, T, J, X.shape[1], Ko, False, site, obs)["D"]
    rng = np.random.default_rng(len(case) + 50)
    for K in (100, int(max(20, np.nanmax(Y)))):
        th = _theta(rng, D, X.shape[1] + Ko + 2)
        c = A.nmix_cells(X, W, Y, th, K, site_re=site, obs_re=obs)
        lj = oracle.literal_log_joint_nmix(th, X, W, Y, max_abundance=K, site_random_effects=site, obs_random_effects=obs)
        want = lj - log_prior(th, N, T, J, X.shape[1], Ko, False, site, obs)
        assert abs(c["l"].sum() - want) <= 1e-10 * abs(want), (case, K, c["l"].sum(), want)
        assert np.max(np.abs(c["pmf"].sum(-1) - 1.0)) <= 1e-12
        # no mass below the largest count of the cell
        m = ~(np.isnan(Y) | np.isnan(W).any(-1) | np.isnan(X).any(-1)[:, None, None])
        ymax = np.where(m, np.nan_to_num(Y), 0.0).max(-1).T                       # (T, N)
        below = np.arange(K + 1)[None, None, :] < ymax[..., None]
        assert below.any() and np.all(c["pmf"][below] == 0.0)


FIXTURES = [c for c in R.case_names() if R.load(c)["model"] in ("occu_rn", "nmixture") and R.load(c)["dims"]["S"] == 1]


def test_the_fixture_list_covers_both_families():
    assert {"rn_default", "rn_missing", "rn_fp", "rn_re_site", "rn_small_2x2", "priors_rn", "nmix_default", "nmix_ref_test", "nmix_re_site",
            "nmix_small_2x2", "priors_nmix"} <= set(FIXTURES)


@pytest.mark.parametrize("case", FIXTURES)
def test_restatement_reproduces_the_reference_models_potential(case):
    """sum over cells of l = -U_fixture - log prior(theta), to the tolerance tests/test_reference_logjoint.py holds the oracle to."""
    e = R.load(case)
    X, W, Y, kw = R.build(e)
    N, T, J, Ko = W.shape
    Ks = X.shape[1]
    rn = e["model"] == "occu_rn"
    fp, site, obs = bool(kw.get("re_fp_mode")), kw["site_random_effects"], kw["obs_random_effects"]
    K = kw.get("max_abundance", 100)
    for p in e["points"]:
        th = R.flat_theta(e, p["unconstrained"])
        lp = log_prior(th, N, T, J, Ks, Ko, fp, site, obs, kw["prior_beta"], kw["prior_alpha"], kw["prior_family"], kw.get("prior_fp", (2.0, 5.0)),
                       (kw.get("prior_site_re_sd", 1.0), kw.get("prior_obs_re_sd", 1.0)))
        c = A.rn_cells(X, W, Y[0], th, K, fp=fp, site_re=site, obs_re=obs) if rn else A.nmix_cells(X, W, Y[0], th, K, site_re=site, obs_re=obs)
        want = -p["U"] - lp
        assert abs(c["l"].sum() - want) <= 1e-10 * abs(want), (case, p["label"], c["l"].sum(), want)


def _small(rng, counts, N=30, T=2, J=4):
    X, W = rng.normal(size=(N, 2)), rng.normal(size=(N, T, J, 1))
    Y = rng.poisson(1.5, size=(N, T, J)).astype(float) if counts else (rng.uniform(size=(N, T, J)) < 0.3).astype(float)
    Y[rng.uniform(size=Y.shape) < 0.25] = np.nan
    Y[:3] = np.nan                     # sites without any observation
    X[5, 0] = np.nan                   # a site covariate masks the whole site
    W[7, 1, :, 0] = np.nan             # a visit covariate masks its visits: period 1 of site 7 is empty
    return X, W, Y


def test_structure_of_the_rn_cells():
    rng = np.random.default_rng(0)
    X, W, Y = _small(rng, counts=False)
    th = rng.uniform(-1, 1, size=5)
    K = 30
    c = A.rn_cells(X, W, Y, th, K)
    empty = c["n_obs"] == 0
    assert empty[:, :3].all() and empty[:, 5].all() and empty[1, 7] and not empty.all()
    # an empty cell is the prior: likelihood 1, the Poisson pmf renormalised on 0..K
    n = np.arange(K + 1)
    eta = th[0] + np.nan_to_num(X.astype(np.float32).astype(np.float64)) @ th[1:3]
    logits = eta[:, None] * n - gammaln(n + 1)
    prior = np.exp(logits - logsumexp(logits, axis=1, keepdims=True))           # (N, K + 1)
    assert np.max(np.abs(c["l"][empty])) <= 1e-14
    assert np.max(np.abs(c["pmf"] - prior[None])[empty]) <= 1e-14
    # a detection without a false-positive rate: N = 0 keeps tiny-scale mass only
    m = ~(np.isnan(Y) | np.isnan(W).any(-1) | np.isnan(X).any(-1)[:, None, None])
    det = ((np.nan_to_num(Y) > 0) & m).any(-1).T
    assert det.sum() > 10 and np.all(c["pmf"][det][:, 0] <= 1e3 * TINY) and np.all(c["occ"][det] >= 1 - 1e-30)
    assert np.all(c["mean"][det] >= 1 - 1e-12)
    non = ~det & ~empty
    assert np.all(c["occ"][non] < 1 - prior[:, 0][None].repeat(2, 0)[non])       # only non-detections: less likely occupied than a priori
    cf = A.rn_cells(X, W, Y, np.r_[th, -1.0], K, fp=True)                         # with a rate a detection no longer proves N > 0
    assert np.all(cf["pmf"][det][:, 0] > 1e-6) and np.max(np.abs(cf["l"][empty])) <= 1e-14
    # random effects enter through their offsets: zero effects change nothing
    o = occu_theta_layout(30, 2, 4, 2, 1, False, True, True)
    thr = np.r_[th, 0.3, -0.2, np.zeros(o["D"] - 7)]
    cr = A.rn_cells(X, W, Y, thr, K, site_re=True, obs_re=True)
    assert np.allclose(cr["l"], c["l"], rtol=0, atol=1e-13)
    thr[o["u"] + 9] = 1.0
    cr = A.rn_cells(X, W, Y, thr, K, site_re=True, obs_re=True)
    assert np.all(cr["mean"][:, 9] > c["mean"][:, 9]) and np.allclose(np.delete(cr["l"], 9, axis=1), np.delete(c["l"], 9, axis=1), rtol=0, atol=1e-13)


def test_structure_of_the_nmix_cells():
    rng = np.random.default_rng(1)
    X, W, Y = _small(rng, counts=True)
    th = np.r_[3.0, rng.uniform(-0.3, 0.3, size=4)]   # lambda near K: the cut at K takes visible mass
    K = 25
    c = A.nmix_cells(X, W, Y, th, K)
    empty = c["n_obs"] == 0
    assert empty[:, :3].all() and empty[1, 7] and not empty.all()
    lam = np.exp(th[0] + np.nan_to_num(X.astype(np.float32).astype(np.float64)) @ th[1:3])
    log_cdf = stats.poisson.logcdf(K, lam)                                      # log P(N <= K): not zero
    want = np.broadcast_to(log_cdf[None], c["l"].shape)
    assert np.max(np.abs(c["l"] - want)[empty]) <= 1e-12 and np.all(c["l"][empty] < 0)
    prior = stats.poisson.pmf(np.arange(K + 1)[None], lam[:, None]) / np.exp(log_cdf)[:, None]
    assert np.max(np.abs(c["pmf"] - prior[None])[empty]) <= 1e-13
    m = ~(np.isnan(Y) | np.isnan(W).any(-1) | np.isnan(X).any(-1)[:, None, None])
    ymax = np.where(m, np.nan_to_num(Y), 0.0).max(-1).T
    assert np.all(c["mean"] >= ymax - 1e-12) and np.all(c["occ"][ymax > 0] == 1.0)
    bl, bm, bo = A.bounds(c, 2e-6)
    assert bl.shape == bm.shape == bo.shape == c["l"].shape and np.all(bl > 0) and np.all(bm > 0) and np.all(bo >= 2.0 ** -23)


def test_criteria_on_a_hand_made_result():
    rng = np.random.default_rng(2)
    n, T, N, S = 6, 2, 5, 2
    ll = -rng.gamma(2.0, size=(n, T, N, S)).astype(np.float32)
    n_obs = rng.integers(0, 3, size=(T, N, S)).astype(np.int32)
    n_obs[0, 0, 0] = 0
    Ni = rng.poisson(2.0, size=(n, T, N, S)).astype(np.int32)
    lat = dict(log_lik=ll, n_obs=n_obs, N_i=Ni)
    fs = finite_sample_abundance(lat)
    assert fs.shape == (n, T, S) and fs.dtype == np.float64 and np.array_equal(fs, Ni.sum(axis=2))
    col = ll.astype(np.float64)[:, n_obs > 0]
    lppd = float(np.sum(logsumexp(col, axis=0) - np.log(n)))
    p = float(np.sum(np.var(col, axis=0, ddof=1)))
    w = waic_marginal(lat)
    assert abs(lppd_marginal(lat) - lppd) <= 1e-12 * abs(lppd)
    assert abs(w["lppd"] - lppd) <= 1e-12 * abs(lppd) and abs(w["p_waic"] - p) <= 1e-12 * p and abs(w["waic"] + 2 * (lppd - p)) <= 1e-10


def test_python_refusals():
    with pytest.raises(TypeError):
        conditional_abundance(lambda **kw: None, None)
    with pytest.raises(TypeError):
        conditional_abundance("occu_rn", None)
    for name in ("occu", "occu_comb", "occu_cop", "occu_cs", "occu_dyn"):
        with pytest.raises(NotImplementedError, match=name):
            conditional_abundance(getattr(models, name), None)
    for name in ("occu", "occu_comb"):
        with pytest.raises(NotImplementedError, match="conditional_occupancy"):
            conditional_abundance(getattr(models, name), None)


@pytest.mark.skipif(_ffi.device_count() > 0, reason="only meaningful on a box without a GPU (tests/test_gpu_abundance.py runs the call)")
def test_no_fallback_without_a_device():
    """Without a GPU conditional_abundance raises the engine's error: there is no host path."""
    X, W, Y = _sim(simulate_rn, n_sites=20, deployment_days_per_site=28)

    class _Mcmc:
        def get_samples(self):
            return dict(beta=np.zeros((3, 1, 2), dtype=np.float32), alpha=np.zeros((3, 1, 2), dtype=np.float32))

    with pytest.raises(_ffi.EngineError, match="no HIP device"):
        conditional_abundance(models.occu_rn, _Mcmc(), site_covs=X, obs_covs=W, obs=Y[None])
