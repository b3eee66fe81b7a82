"""Conditional counts of occu_cop in float64 NumPy (TEST INFRASTRUCTURE): what ``bl_count_posterior`` returns, restated replicate by
replicate from the reference's model (biolith/models/occu_cop.py:150-255), independent of the kernel:

    z ~ Bernoulli(psi);  y_j ~ Poisson(d_j (z lambda_j + (1 - z) f_u + f_c)),  lambda_j = exp(nu_j), masked where the count, one of the
    visit's covariates or one of the site's covariates is missing (NaN covariates read as 0).

With f the sampled rate (0 without one), f1 = f in "constant" mode else 0, f0 = f, c_j = y_j log d_j - lgamma(y_j + 1):
A = log psi + sum_j [y_j log(lambda_j + f1) - d_j (lambda_j + f1) + c_j], B = log(1 - psi) + sum_j [y_j log f0 - d_j f0 + c_j] (f0 = 0:
the Poisson(0) pmf, 0 or -inf), l = logaddexp(A, B), q = exp(A - l).  lambda_j = exp(min(nu_j, 80)) and f = exp(min(phi, 80)) are the
sampler's clamps (never reached by a test's theta).  Given z = 1 and y_j, the real detections are Binomial(y_j, rho_j) with rho_j =
lambda_j / (lambda_j + f1) (Poisson thinning), given z = 0 there are none: true_mean_j = q y_j rho_j.

``cop_cells`` returns a dict: per cell, (T, N) float64, A, B, l, q, psi, n_obs, y_sum, S_A, S_B, S as tests/latent_ref.py (S_*: sums of
the absolute values of a branch's terms: |log psi|, and per unmasked visit |y log(lambda + f1)|, |d (lambda + f1)| and |c_j|; for B
|y log f0|, |d f0|, |c_j|); per visit, (J, T, N): ``m`` the mask, ``y`` (0 where masked), ``rho``, ``true_mean`` and ``S_v`` = |nu_j| + |phi|,
the absolute values of the two terms of logit rho_j = nu_j - phi (0 where rho_j = 1 by construction).

``bounds`` follows tests/latent_ref.py: bounds.  log_lik: rtol S + ulp32(l) / 2.  z_prob = sigmoid(A - B): (bound on A + bound on B) / 4
+ 2^-23; where B = -inf (no rate, a positive count) q is 1 and B has no allowance.  true_mean_j = y_j sigmoid(A - B) sigmoid(nu_j - phi):
the same formula with S_A + S_v in the place of S_A, scaled by y_j.
"""
import math

import numpy as np
from scipy import stats
from scipy.special import gammaln

import latent_ref as L


def _log_sigmoid(x):
    return -np.logaddexp(0.0, -x)


def cop_cells(site_covs, obs_covs, counts, session_duration, th, fp_mode=None, site_re=False, obs_re=False):
    """site_covs (N, Ks), obs_covs (N, T, J, Ko), counts and session_duration (N, T, J) of ONE species (NaN = missing), th the
    engine's flat coordinates [beta, alpha, (phi = log rate), (log sds), (site_re_occ [N], site_re_det [N]), (obs_re [N][T][J])]."""
    X, W, Y, Dur = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (site_covs, obs_covs, counts, session_duration))
    th = np.asarray(th, dtype=np.float64)
    N, T, J, Ko = W.shape
    Ks = X.shape[1]
    o = L.occu_theta_layout(N, T, J, Ks, Ko, fp_mode is not None, site_re, obs_re)
    assert th.shape == (o["D"],), (th.shape, o["D"])
    assert fp_mode in (None, "constant", "unoccupied")
    m = ~(~np.isfinite(Y) | np.isnan(W).any(-1) | np.isnan(X).any(-1)[:, None, None])          # (N, T, J)
    X, W, Y = np.nan_to_num(X), np.nan_to_num(W), np.where(m, np.nan_to_num(Y), 0.0)
    beta, alpha = th[:Ks + 1], th[Ks + 1:Ks + Ko + 2]
    eta = beta[0] + X @ beta[1:] + (th[o["u"]:o["u"] + N] if site_re else 0.0)
    lpsi, l1psi = _log_sigmoid(eta), _log_sigmoid(-eta)
    phi = th[o["fp"]] if fp_mode is not None else -np.inf
    f = math.exp(min(phi, 80.0)) if fp_mode is not None else 0.0
    f1 = f if fp_mode == "constant" else 0.0
    A, B = np.repeat(lpsi[:, None], T, 1), np.repeat(l1psi[:, None], T, 1)
    SA, SB = np.abs(A), np.abs(B)
    rho, Sv = np.ones((N, T, J)), np.zeros((N, T, J))
    for j in range(J):
        nu = alpha[0] + W[:, :, j] @ alpha[1:]
        if site_re:
            nu = nu + th[o["v"]:o["v"] + N][:, None]
        if obs_re:
            nu = nu + th[o["e"]:o["e"] + N * T * J].reshape(N, T, J)[:, :, j]
        nu = np.minimum(nu, 80.0)
        lam = np.exp(nu)
        y, d, mj = Y[:, :, j], Dur[:, :, j], m[:, :, j]
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where(mj, np.where(y > 0, y * np.log(d), 0.0) - gammaln(y + 1.0), 0.0)
        log_rate = np.log(lam + f1) if f1 > 0 else nu                     # log(lambda) is nu itself
        t1, t2 = y * log_rate, d * (lam + f1)
        A = A + np.where(mj, t1 - t2 + c, 0.0)
        SA = SA + np.where(mj, np.abs(t1) + np.abs(t2) + np.abs(c), 0.0)
        if fp_mode is not None:
            b1, b2 = y * phi, d * f
            B = B + np.where(mj, b1 - b2 + c, 0.0)
            SB = SB + np.where(mj, np.abs(b1) + np.abs(b2) + np.abs(c), 0.0)
        else:                                                              # Poisson(0): 0 at a zero count, -inf at a positive one
            B = B + np.where(mj, np.where(y > 0, -np.inf, c), 0.0)
            SB = SB + np.where(mj, np.abs(c), 0.0)
        if f1 > 0:
            rho[:, :, j] = lam / (lam + f1)
            Sv[:, :, j] = np.abs(nu) + abs(phi)
    n_obs = m.sum(-1)
    l, psi = np.logaddexp(A, B), np.repeat(np.exp(lpsi)[:, None], T, 1)
    q = np.exp(A - l)
    l, q = np.where(n_obs == 0, 0.0, l), np.where(n_obs == 0, psi, q)   # (what the formulas give there, stated exactly)
    cell = dict(A=A, B=B, l=l, q=q, psi=psi, n_obs=n_obs, y_sum=Y.sum(-1), S_A=SA, S_B=SB, S=SA + SB)
    out = {k: np.ascontiguousarray(v.T) for k, v in cell.items()}                                            # (N, T) -> (T, N)
    visit = dict(m=m, y=Y, rho=np.where(m, rho, 1.0), true_mean=np.where(m, q[:, :, None] * Y * rho, 0.0), S_v=np.where(m, Sv, 0.0))
    out.update({k: np.ascontiguousarray(v.transpose(2, 1, 0)) for k, v in visit.items()})                    # (N, T, J) -> (J, T, N)
    return out


def bounds(c, rtol):
    """(on log_lik (T, N), on z_prob (T, N), on true_mean (J, T, N)): see the module docstring."""
    dead = np.isneginf(c["B"])
    B = np.where(dead, 0.0, c["B"])
    bl = rtol * c["S"] + 0.5 * L.ulp32(c["l"])
    bB = np.where(dead, 0.0, rtol * c["S_B"] + 0.5 * L.ulp32(B))
    bA = rtol * c["S_A"] + 0.5 * L.ulp32(c["A"])
    bq = 0.25 * (bA + bB) + 2.0 ** -23
    bt = c["y"] * (0.25 * (rtol * (c["S_A"][None] + c["S_v"]) + 0.5 * L.ulp32(c["A"])[None] + bB[None]) + 2.0 ** -23)
    return bl, bq, bt


def log_prior(th, N, T, J, Ks, Ko, fp_mode=None, site_re=False, obs_re=False, prior_beta=(0.0, 1.0), prior_alpha=(0.0, 1.0),
              prior_fp_rate=1.0, sd_scales=(1.0, 1.0)):
    """log prior of the engine's coordinates with scipy.stats: Normal coefficients; rate ~ Exponential(prior_fp_rate) in phi = log rate
    (+ phi, the Jacobian); sd ~ HalfNormal(scale) in log sd (+ log sd); the effects Normal(0, sd)."""
    th = np.asarray(th, dtype=np.float64)
    o = L.occu_theta_layout(N, T, J, Ks, Ko, fp_mode is not None, site_re, obs_re)
    lp = float(np.sum(stats.norm.logpdf(th[:Ks + 1], *prior_beta)) + np.sum(stats.norm.logpdf(th[Ks + 1:Ks + Ko + 2], *prior_alpha)))
    at = Ks + Ko + 2
    if fp_mode is not None:
        lp += float(stats.expon.logpdf(math.exp(th[at]), scale=1.0 / prior_fp_rate)) + th[at]
        at += 1
    sds = []
    for on, sc in ((site_re, sd_scales[0]), (obs_re, sd_scales[1])):
        if on:
            lp += float(stats.halfnorm.logpdf(math.exp(th[at]), scale=sc)) + th[at]
            sds.append(math.exp(th[at]))
            at += 1
    if site_re:
        lp += float(np.sum(stats.norm.logpdf(th[o["u"]:o["u"] + 2 * N], 0.0, sds[0])))
    if obs_re:
        lp += float(np.sum(stats.norm.logpdf(th[o["e"]:o["e"] + N * T * J], 0.0, sds[-1])))
    return lp


def make_data(rng, N, T, J, Ks, Ko, missing=0.3):
    """Counts up to a few dozen (four cells in ten all zero), durations in [0.5, 3], ``missing`` of the counts NaN, site 0 without any
    count, a NaN site covariate at site 5 and a NaN observation covariate at site 7 (where the model has covariates).
    Returns X (N, Ks), W (N, T, J, Ko), Y (N, T, J), Dur (N, T, J) as float32."""
    X, W = rng.normal(size=(N, Ks)), rng.normal(size=(N, T, J, Ko))
    Dur = rng.uniform(0.5, 3.0, size=(N, T, J))
    Y = rng.poisson(rng.uniform(0.0, 12.0, size=(N, T, J)) * (rng.uniform(size=(N, T, 1)) > 0.4)).astype(float)
    Y[rng.uniform(size=Y.shape) < missing] = np.nan
    Y[0] = np.nan
    if Ks:
        X[5, 0] = np.nan
    if Ko:
        W[7, 0, 1, 0] = np.nan
    return tuple(a.astype(np.float32) for a in (X, W, Y, Dur))


def frequency_case():
    """The inputs of the draw-frequency tests (tests/test_counts_cpu.py, tests/test_gpu_counts.py): 850 sites x 2 periods x 10 visits,
    "constant" mode, short sessions and detection rates of the order of the false-positive rate, so that many cells are undecided and
    many counted detections may or may not be real; 45 % of the counts missing.  One theta, and the number of times the draw is
    repeated on the device -- 4000 draws of 68 kB of true_mean each, a little more than one 256 MB chunk of the entry's device scratch.
    Returns X, W, Y (N, T, J), Dur, theta, n."""
    rng = np.random.default_rng(11)
    N, T, J = 850, 2, 10
    X, W = rng.normal(size=(N, 1)), rng.normal(size=(N, T, J, 1))
    Dur = rng.uniform(0.5, 3.0, size=(N, T, J))
    th = np.array([0.1, 0.6, -0.9, 0.5, math.log(0.35)])
    psi = 1 / (1 + np.exp(-(th[0] + th[1] * X[:, 0])))
    z = rng.uniform(size=(N, T)) < psi[:, None]
    lam = np.exp(th[2] + th[3] * W[..., 0])
    Y = rng.poisson(Dur * (z[..., None] * lam + 0.35)).astype(float)
    Y[rng.uniform(size=Y.shape) < 0.45] = np.nan
    X, W, Y, Dur = (a.astype(np.float32) for a in (X, W, Y, Dur))
    return X, W, Y, Dur, th.astype(np.float32).astype(np.float64), 4000


def pooled_statistics(c, z_count, t_count, n, z_prob=None, true_mean=None, lo=0.05, hi=0.95):
    """Standardised sums of (z - z_prob) over the cells with q in (lo, hi) and of (true_count - true_mean) over the unmasked visits
    with a positive count and q rho_j in (lo, hi), for n joint draws at the theta of ``c`` (``cop_cells``' result); ``z_count`` (T, N)
    and ``t_count`` (J, T, N) are the draws' sums, ``z_prob`` / ``true_mean`` what they are held against (default: the restatement's
    own).  The z of different cells are independent Bernoulli(q).  The true counts of ONE cell are not independent: true_count_j =
    z K_j with K_j ~ Binomial(y_j, rho_j) independent, so a cell's sum over its selected visits has the variance
    q sum_j y_j rho_j (1 - rho_j) + q (1 - q) (sum_j y_j rho_j)^2; standardising by the binomial variances alone would be too narrow by
    the second term.  Returns {"z": (stat, count), "t": (stat, count)}."""
    q, rho, y = c["q"], c["rho"], c["y"]
    zp = q if z_prob is None else np.asarray(z_prob, dtype=np.float64)
    tm = c["true_mean"] if true_mean is None else np.asarray(true_mean, dtype=np.float64)
    mz = (q > lo) & (q < hi) & (c["n_obs"] > 0)
    stat_z = float((z_count[mz] - n * zp[mz]).sum() / np.sqrt(n * (q[mz] * (1 - q[mz])).sum()))
    mt = c["m"] & (y > 0) & (q[None] * rho > lo) & (q[None] * rho < hi)
    mean_j, var_j = np.where(mt, y * rho, 0.0), np.where(mt, y * rho * (1 - rho), 0.0)
    var = q * var_j.sum(0) + q * (1 - q) * mean_j.sum(0) ** 2                                  # per cell
    stat_t = float((t_count[mt] - n * tm[mt]).sum() / np.sqrt(n * var.sum()))
    return {"z": (stat_z, int(mz.sum())), "t": (stat_t, int(mt.sum()))}
