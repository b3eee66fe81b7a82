"""Conditional occupancy without a GPU: the float64 restatement (tests/latent_ref.py) pinned to the densities the project already
trusts, its structure, the host-side criteria (lppd_marginal / waic_marginal / finite_sample_occupancy) and the Python refusals."""
import numpy as np
import pytest
from scipy import stats
from scipy.special import logsumexp

import latent_ref as L
import reference_logjoint as R
from biolith_amd import models
from biolith_amd.evaluation import finite_sample_occupancy, lppd_marginal, waic_marginal
from biolith_amd.utils import conditional_occupancy
from comb_ref import REF_INDEX, CombRef, reference_case

# the committed plain-occu and false-positive fixtures of the reference's own model (one species, no random effects)
OCCU_CASES = [c for c in R.case_names()
              if (lambda e: e["model"] == "occu" and e["dims"]["S"] == 1 and not e["model_kwargs"].get("site_random_effects")
                  and not e["model_kwargs"].get("obs_random_effects"))(R.load(c))]


def test_the_case_list_covers_plain_and_false_positive_fixtures():
    assert {"default", "missing", "missing_3periods", "small_3x3", "fp_constant", "fp_unoccupied", "priors_normal", "priors_laplace",
            "priors_fp"} <= set(OCCU_CASES)


def _coef_logprior(x, prior, family):
    dist = stats.laplace if family == "laplace" else stats.norm
    return float(np.sum(dist.logpdf(x, loc=prior[0], scale=prior[1])))


@pytest.mark.parametrize("case", OCCU_CASES)
def test_restatement_sums_to_the_reference_models_likelihood(case):
    """sum over cells of l = -U_fixture - log prior(theta): the priors and the logit Jacobian of the rate restated with scipy.stats."""
    e = R.load(case)
    X, W, Y, kw = R.build(e)
    Ks, Ko = X.shape[1], W.shape[3]
    fp = kw.get("fp_mode") if kw["model"] == "occu_fp" else None
    for p in e["points"][:4]:   # (the fifth is the clamp regime, the oracle's one documented deviation: test_reference_logjoint.py)
        th = R.flat_theta(e, p["unconstrained"])
        lp = _coef_logprior(th[:Ks + 1], kw["prior_beta"], kw["prior_family"][0]) + _coef_logprior(th[Ks + 1:Ks + Ko + 2], kw["prior_alpha"], kw["prior_family"][1])
        if fp is not None:
            a, b = kw.get("prior_fp", (2.0, 5.0))
            f = 1.0 / (1.0 + np.exp(-th[-1]))
            lp += float(stats.beta.logpdf(f, a, b) + np.log(f) + np.log1p(-f))   # d f / d phi = f (1 - f)
        c = L.occu_cells(X, W, Y[0], th, fp_mode=fp)
        want = -p["U"] - lp
        assert abs(c["l"].sum() - want) <= 1e-10 * abs(want), (case, p["label"], c["l"].sum(), want)


@pytest.mark.parametrize("case", sorted(REF_INDEX))
def test_comb_restatement_sums_to_comb_ref(case):
    data, pri, fx = reference_case(case)
    ref = CombRef(data["site_covs"], data["PC_obs_covs"], data["ARU_obs_covs"], data["PC_obs"][:1], data["ARU_obs"][:1],
                  data["scores_obs"][:1], **pri)
    assert len(sorted(REF_INDEX)) == 5
    for p in fx["points"]:
        th = np.asarray(p["theta"], dtype=np.float64)
        c = L.comb_cells(ref, th)
        want = ref.log_lik(th)
        assert abs(c["l"].sum() - want) <= 1e-10 * abs(want), (case, c["l"].sum(), want)
        assert c["l"].shape == (ref.Yp.shape[1], ref.Yp.shape[0])


def _occu_data(rng, N=40, T=2, J=4, Ks=2, Ko=2):
    X, W = rng.normal(size=(N, Ks)), rng.normal(size=(N, T, J, Ko))
    Y = (rng.uniform(size=(N, T, J)) < 0.3).astype(float)
    Y[rng.uniform(size=Y.shape) < 0.25] = np.nan
    Y[:3] = np.nan                     # sites without any observation
    X[5, 0] = np.nan                   # a site covariate masks the whole site
    W[7, 1, :, 1] = np.nan             # a visit covariate masks its visits: period 1 of site 7 is empty
    return X, W, Y


def test_structure_of_the_cells():
    rng = np.random.default_rng(0)
    X, W, Y = _occu_data(rng)
    th = rng.uniform(-1.5, 1.5, size=6)
    c = L.occu_cells(X, W, Y, th)
    empty = c["n_obs"] == 0
    assert empty[:, :3].all() and empty[:, 5].all() and empty[1, 7] and not empty.all()
    assert np.max(np.abs(c["l"][empty])) <= 1e-15 and np.max(np.abs(c["q"][empty] - c["psi"][empty])) <= 1e-15
    det = (np.nan_to_num(Y) > 0).any(-1).T & ~empty   # (T, N); Y's NaN sites are empty anyway
    det &= ~np.isnan(X).any(-1)[None]
    assert det.sum() > 10 and (c["q"][det] >= 1 - 1e-30).all()
    assert (c["q"][~det & ~empty] < c["psi"][~det & ~empty]).all()   # only non-detections: less likely occupied than a priori
    # with a false-positive rate a detection no longer proves occupancy
    for mode in ("constant", "unoccupied"):
        cf = L.occu_cells(X, W, Y, np.r_[th, -1.0], fp_mode=mode)
        assert (cf["q"][det] < 1 - 1e-6).all() and np.max(np.abs(cf["l"][empty])) <= 1e-15
    # random effects enter through their offsets: zero effects change nothing
    o = L.occu_theta_layout(40, 2, 4, 2, 2, False, True, True)
    thr = np.r_[th, 0.3, -0.2, np.zeros(o["D"] - 8)]
    cr = L.occu_cells(X, W, Y, thr, site_re=True, obs_re=True)
    assert np.allclose(cr["l"], c["l"], rtol=0, atol=1e-14)
    thr[o["u"] + 9] = 2.0
    cr = L.occu_cells(X, W, Y, thr, site_re=True, obs_re=True)
    assert np.all(cr["psi"][:, 9] > c["psi"][:, 9]) and np.allclose(np.delete(cr["l"], 9, axis=1), np.delete(c["l"], 9, axis=1), rtol=0, atol=1e-14)


def test_marginal_criteria_against_a_hand_computation():
    rng = np.random.default_rng(1)
    n, T, N, S = 7, 2, 5, 2
    ll = -rng.gamma(2.0, size=(n, T, N, S))
    n_obs = rng.integers(0, 3, size=(T, N, S))
    n_obs[0, 0, 0], n_obs[1, 2, 1] = 0, 0
    ll[:, n_obs == 0] = 0.0
    z = (rng.uniform(size=(n, T, N, S)) < 0.4).astype(np.int32)
    lat = dict(log_lik=ll.astype(np.float32), n_obs=n_obs.astype(np.int32), z=z)
    lppd = p = 0.0
    for t in range(T):
        for i in range(N):
            for s in range(S):
                if n_obs[t, i, s] == 0:
                    continue
                col = ll.astype(np.float32).astype(np.float64)[:, t, i, s]
                lppd += logsumexp(col) - np.log(n)
                p += np.var(col, ddof=1)
    assert abs(lppd_marginal(lat) - lppd) <= 1e-12 * abs(lppd)
    w = waic_marginal(lat)
    assert set(w) == {"waic", "p_waic", "lppd"}
    assert abs(w["lppd"] - lppd) <= 1e-12 * abs(lppd) and abs(w["p_waic"] - p) <= 1e-12 * p and abs(w["waic"] + 2 * (lppd - p)) <= 1e-10
    # the excluded cells really are excluded: garbage there changes nothing
    lat2 = dict(lat, log_lik=np.where(n_obs == 0, -1e6, lat["log_lik"]).astype(np.float32))
    assert waic_marginal(lat2) == w
    fs = finite_sample_occupancy(lat)
    assert fs.shape == (n, T, S) and np.allclose(fs, z.mean(axis=2))
    with pytest.raises(ValueError):
        lppd_marginal(dict(log_lik=ll, n_obs=n_obs[:1]))


def test_python_refusals():
    with pytest.raises(TypeError):
        conditional_occupancy(lambda **kw: None, None)
    with pytest.raises(TypeError):
        conditional_occupancy("occu", None)
    for name in ("occu_rn", "nmixture", "occu_cop", "occu_cs", "occu_dyn"):
        with pytest.raises(NotImplementedError, match=name):
            conditional_occupancy(getattr(models, name), None)
