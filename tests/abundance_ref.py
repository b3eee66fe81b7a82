"""Conditional abundance in float64 NumPy (TEST INFRASTRUCTURE): per (period, site) cell the addends of the N-marginalised likelihood,
l_n for n = 0..K, their logsumexp ``l``, the conditional pmf exp(l_n - l), its mean, sd and 1 - pmf(0), for the two families
``bl_abundance_posterior`` serves -- written from the model text, with the clamps and masks of the densities the project already trusts
(``oracle.literal_log_joint_rn`` / ``_nmix``; tests/test_abundance_cpu.py pins the cells' sums to them and to the reference fixtures):

occu_rn   l_n = [n log lambda - lgamma(n + 1) - lambda] - logsumexp_m [..] + sum_j log Bernoulli(y_j; clip(1 - (1 - p_nj)(1 - f))),
          p_nj = 1 - (1 - r_j)^n, the clip to [float32 tiny, 1 - float32 eps] being numpyro's; f the false-positive rate or 0.
nmixture  l_n = n log lambda - lgamma(n + 1) - lambda + sum_j [log C(n, y_j) + y_j log p_j + (n - y_j) log(1 - p_j)] for
          max_j y_j <= n <= K and -inf below: the untruncated Poisson cut at K (the model's N_i_trunc_norm factor times its
          normalising Categorical).
A visit is masked where y, one of its covariates or a site covariate is NaN.

Each function returns a dict of float64 arrays per (T, N): ``l``, ``pmf`` (T, N, K + 1), ``mean``, ``occ`` = 1 - pmf(0), ``sd``, ``n_obs``
and the scale ``S`` = sum_n pmf(n) S_n with S_n the sum of the absolute values of the terms of l_n as listed above (each Poisson piece,
the normaliser, every visit's log-probability; for the Binomial its three pieces).

Bounds of a float32 evaluation against this restatement (``bounds``), derived, not measured:
log_lik   every term of l_n carries a relative error of some ulps, so l_n is off by d_n <= rtol S_n; l = logsumexp_n l_n has
          dl / dl_n = pmf(n), hence |error| <= sum_n pmf(n) rtol S_n = rtol S, plus half an ulp for rounding l itself to float32.
N_mean    d mean / d l_n = pmf(n) (n - mean), so |error| <= d sum_n pmf(n) |n - mean| <= d sd (Jensen: E|n - mean| <= sd) with d the
          allowance of log_lik, plus one ulp of the mean for forming and rounding the quotient.
occ_prob  = 1 - pmf(0): d / d l_0 = -pmf(0) (1 - pmf(0)), d / d l_n = pmf(0) pmf(n), in total at most 2 pmf(0) (1 - pmf(0)) d <= d / 2,
          plus one ulp of 1 (2^-23).
"""
import math

import numpy as np
from scipy import stats
from scipy.special import gammaln, logsumexp, xlog1py, xlogy

from latent_ref import occu_theta_layout, ulp32

TINY, EPS = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).eps)


def _predictors(site_covs, obs_covs, obs, th, fp, site_re, obs_re):
    X, W, Y = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (site_covs, obs_covs, obs))
    th = np.asarray(th, dtype=np.float64)
    N, T, J, Ko = W.shape
    Ks = X.shape[1]
    o = occu_theta_layout(N, T, J, Ks, Ko, fp, site_re, obs_re)   # [beta, alpha, (phi), (log sds), u [N], v [N], e [N][T][J]]
    assert th.shape == (o["D"],), (th.shape, o["D"])
    m = ~(np.isnan(Y) | np.isnan(W).any(-1) | np.isnan(X).any(-1)[:, None, None])          # (N, T, J)
    X, W, Y = np.nan_to_num(X), np.nan_to_num(W), np.nan_to_num(Y)
    beta, alpha = th[:Ks + 1], th[Ks + 1:Ks + Ko + 2]
    eta = beta[0] + X @ beta[1:] + (th[o["u"]:o["u"] + N] if site_re else 0.0)
    nu = alpha[0] + W @ alpha[1:]
    if site_re:
        nu = nu + th[o["v"]:o["v"] + N][:, None, None]
    if obs_re:
        nu = nu + th[o["e"]:o["e"] + N * T * J].reshape(N, T, J)
    return eta, nu, Y, m, (th[o["fp"]] if fp else None)


def _finish(ln, Sn, m):
    """ln, Sn (N, T, K + 1), m (N, T, J) -> the cell dict, (T, N) first."""
    support = np.arange(ln.shape[-1], dtype=np.float64)
    l = logsumexp(ln, axis=-1)
    pmf = np.exp(ln - l[..., None])
    mean = (pmf * support).sum(-1)
    sd = np.sqrt((pmf * (support - mean[..., None]) ** 2).sum(-1))
    S = np.where(pmf > 0, pmf * np.where(np.isfinite(Sn), Sn, 0.0), 0.0).sum(-1)
    out = dict(l=l, mean=mean, occ=1.0 - pmf[..., 0], sd=sd, n_obs=m.sum(-1), S=S)
    out = {k: np.ascontiguousarray(np.asarray(v).T) for k, v in out.items()}   # (N, T) -> (T, N)
    out["pmf"] = np.ascontiguousarray(pmf.transpose(1, 0, 2))
    return out


def rn_cells(site_covs, obs_covs, obs, th, max_abundance=100, fp=False, site_re=False, obs_re=False):
    """site_covs (N, Ks), obs_covs (N, T, J, Ko), obs (N, T, J) of ONE species (NaN = missing), th the engine's flat coordinates
    [beta, alpha, (logit f), (log site sd), (log obs sd), (site_re_abu [N], site_re_det [N]), (obs_re [N][T][J])]."""
    eta, nu, Y, m, phi = _predictors(site_covs, obs_covs, obs, th, fp, site_re, obs_re)
    n = np.arange(max_abundance + 1, dtype=np.float64)
    lam = np.exp(eta)
    pieces = [eta[:, None] * n, -gammaln(n + 1.0)[None, :] + 0.0 * eta[:, None], -lam[:, None] + 0.0 * n]   # Poisson(lambda).log_prob(n)
    logits = pieces[0] + pieces[1] + pieces[2]
    lz = logsumexp(logits, axis=1, keepdims=True)                                                        # Categorical renormalises
    log_prior = logits - lz
    S_prior = sum(np.abs(p) for p in pieces) + np.abs(lz)
    f = 0.0 if phi is None else 1.0 / (1.0 + np.exp(-phi))
    lq = -np.logaddexp(0.0, nu)                                    # log(1 - r)
    p = -np.expm1(lq[..., None] * n)                               # 1 - (1 - r)^n   (N, T, J, K + 1)
    p = np.clip(1.0 - (1.0 - p) * (1.0 - f), TINY, 1.0 - EPS)
    ly = np.where(m[..., None], np.where(Y[..., None] > 0, np.log(p), np.log1p(-p)), 0.0)
    ln = log_prior[:, None, :] + ly.sum(2)
    Sn = S_prior[:, None, :] + np.abs(ly).sum(2)
    return _finish(ln, Sn, m)


def nmix_cells(site_covs, obs_covs, obs, th, max_abundance=100, site_re=False, obs_re=False):
    """As ``rn_cells`` for the N-mixture model: obs holds counts."""
    eta, nu, Y, m, _ = _predictors(site_covs, obs_covs, obs, th, False, site_re, obs_re)
    n = np.arange(max_abundance + 1, dtype=np.float64)
    lam = np.exp(eta)
    pieces = [xlogy(n[None, :], lam[:, None]), -gammaln(n + 1.0)[None, :] + 0.0 * eta[:, None], -lam[:, None] + 0.0 * n]
    pois = pieces[0] + pieces[1] + pieces[2]                       # (N, K + 1)
    S_pois = sum(np.abs(p) for p in pieces)
    ymax = np.where(m, Y, 0.0).max(-1)                             # (N, T); 0 where nothing is observed
    pr = 1.0 / (1.0 + np.exp(-nu))
    yy, pp, nn = Y[..., None], pr[..., None], n[None, None, None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        parts = [gammaln(nn + 1.0) - gammaln(yy + 1.0) - gammaln(nn - yy + 1.0), xlogy(yy, pp), xlog1py(nn - yy, -pp)]
    ok = m[..., None] & (nn >= yy)
    lb = sum(np.where(ok, q, 0.0) for q in parts).sum(2)            # (N, T, K + 1)
    Sb = sum(np.where(ok, np.abs(q), 0.0) for q in parts).sum(2)
    feasible = n[None, None, :] >= ymax[..., None]
    ln = np.where(feasible, pois[:, None, :] + lb, -np.inf)
    Sn = np.where(feasible, S_pois[:, None, :] + Sb, 0.0)
    return _finish(ln, Sn, m)


def log_prior(th, N, T, J, Ks, Ko, fp=False, site=False, obs=False, prior_beta=(0.0, 1.0), prior_alpha=(0.0, 1.0),
              family=("normal", "normal"), prior_fp=(2.0, 5.0), sd_scales=(1.0, 1.0)):
    """log prior density of the engine's coordinates, restated with scipy.stats: the coefficients, the Beta rate on the logit scale
    (+ log f (1 - f)), the HalfNormal sds on the log scale (+ log sd), the Normal(0, sd) effects."""
    th = np.asarray(th, dtype=np.float64)
    o = occu_theta_layout(N, T, J, Ks, Ko, fp, site, obs)
    dist = [stats.laplace if f == "laplace" else stats.norm for f in family]
    lp = float(np.sum(dist[0].logpdf(th[:Ks + 1], *prior_beta)) + np.sum(dist[1].logpdf(th[Ks + 1:Ks + Ko + 2], *prior_alpha)))
    at = Ks + Ko + 2
    if fp:
        f = 1.0 / (1.0 + math.exp(-th[at]))
        lp += float(stats.beta.logpdf(f, *prior_fp) + math.log(f) + math.log1p(-f))
        at += 1
    sds = []
    for on, sc in ((site, sd_scales[0]), (obs, sd_scales[1])):
        if on:
            lp += float(stats.halfnorm.logpdf(math.exp(th[at]), scale=sc)) + th[at]
            sds.append(math.exp(th[at]))
            at += 1
    if site:
        lp += float(np.sum(stats.norm.logpdf(th[o["u"]:o["u"] + 2 * N], 0.0, sds[0])))
    if obs:
        lp += float(np.sum(stats.norm.logpdf(th[o["e"]:o["e"] + N * T * J], 0.0, sds[-1])))
    return lp


def bounds(c, rtol):
    """The float32 kernel's allowance per cell against this restatement: (on log_lik, on N_mean, on occ_prob); derivations above."""
    bl = rtol * c["S"] + 0.5 * ulp32(c["l"])
    return bl, bl * c["sd"] + ulp32(c["mean"]), 0.5 * bl + 2.0 ** -23
