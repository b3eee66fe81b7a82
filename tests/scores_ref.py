"""Conditional scores of occu_cs in float64 NumPy (TEST INFRASTRUCTURE): what ``bl_score_posterior`` returns, restated visit by visit
from the reference's model (biolith/models/occu_cs.py:185-223), independent of the kernel:

    z ~ Bernoulli(psi);  f_j ~ Bernoulli(z p_j);  s_j ~ Normal((1 - f_j) mu0 + f_j mu1, (1 - f_j) sigma0 + f_j sigma1), masked where the
    score, one of the visit's covariates or one of the site's covariates is missing (NaN covariates read as 0).

Summing f_j out of an unmasked visit gives p(s_j | z = 1) = p_j N1_j + (1 - p_j) N0_j and p(s_j | z = 0) = N0_j; summing z out of a
cell gives logaddexp(A, B) with A = log psi + sum_j mix_j, B = log(1 - psi) + sum_j n0_j.  Given z = 1, P(f_j = 1 | s_j) =
p_j N1_j / (p_j N1_j + (1 - p_j) N0_j) = exp(log p_j + n1_j - mix_j); a masked visit has no score: P(f_j = 1 | z = 1) = p_j.  All logs of
probabilities are exact log-sigmoids; no clamp.

``cs_cells`` returns a dict: per cell, (T, N) float64, A, B, l, q, psi, n_obs, S_A, S_B, S as tests/latent_ref.py (S_*: sums of the
absolute values of a branch's terms); per visit, (J, T, N): ``m`` the mask, ``p``, ``r`` = P(f_j = 1 | z = 1, s_j), ``f_prob`` = q r and
``S_v``, the sum of the absolute values of the visit's own terms log p_j, n1_j, mix_j (log p_j alone where masked).

``bounds`` follows tests/latent_ref.py: bounds.  log_lik: rtol S + ulp32(l) / 2.  z_prob = exp(A - l) from its two log terms A and B:
(bound on A + bound on B) / 4 + 2^-23.  f_prob_j = exp((A + log p_j + n1_j - mix_j) - l) is the same kind of quantity with the visit's
three terms joining A's: the same formula with S_A + S_v in the place of S_A.
"""
import itertools

import numpy as np

import latent_ref as L

HL2PI = 0.5 * np.log(2 * np.pi)


def _log_sigmoid(x):
    return -np.logaddexp(0.0, -x)


def split(th, Ks, Ko):
    """th = [beta | alpha | mu0 | log(mu1 - mu0) | log sigma0 | log sigma1] -> beta, alpha, mu0, mu1, sigma0, sigma1."""
    th = np.asarray(th, dtype=np.float64)
    assert th.shape == (Ks + Ko + 6,), th.shape
    e = th[Ks + Ko + 2:]
    return th[:Ks + 1], th[Ks + 1:Ks + Ko + 2], e[0], e[0] + np.exp(e[1]), np.exp(e[2]), np.exp(e[3])


def cs_cells(site_covs, obs_covs, scores, th):
    """site_covs (N, Ks), obs_covs (N, T, J, Ko), scores (N, T, J) of the one species (NaN = missing), th the engine's coordinates."""
    X, W, Sc = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (site_covs, obs_covs, scores))
    N, T, J, Ko = W.shape
    beta, alpha, mu0, mu1, sg0, sg1 = split(th, X.shape[1], Ko)
    m = ~(~np.isfinite(Sc) | np.isnan(W).any(-1) | np.isnan(X).any(-1)[:, None, None])          # (N, T, J)
    X, W, Sc = np.nan_to_num(X), np.nan_to_num(W), np.where(np.isfinite(Sc), Sc, 0.0)
    eta = beta[0] + X @ beta[1:]
    lpsi, l1psi = _log_sigmoid(eta), _log_sigmoid(-eta)
    A, B = np.repeat(lpsi[:, None], T, 1), np.repeat(l1psi[:, None], T, 1)
    SA, SB = np.abs(A), np.abs(B)
    p, r, Sv = np.empty((N, T, J)), np.empty((N, T, J)), np.empty((N, T, J))
    for j in range(J):
        nu = alpha[0] + W[:, :, j] @ alpha[1:]
        lp, l1p = _log_sigmoid(nu), _log_sigmoid(-nu)
        n0 = -0.5 * ((Sc[:, :, j] - mu0) / sg0) ** 2 - np.log(sg0) - HL2PI
        n1 = -0.5 * ((Sc[:, :, j] - mu1) / sg1) ** 2 - np.log(sg1) - HL2PI
        mix = np.logaddexp(lp + n1, l1p + n0)
        mj = m[:, :, j]
        A, B = A + np.where(mj, mix, 0.0), B + np.where(mj, n0, 0.0)
        SA, SB = SA + np.where(mj, np.abs(mix), 0.0), SB + np.where(mj, np.abs(n0), 0.0)
        p[:, :, j] = np.exp(lp)
        r[:, :, j] = np.where(mj, np.exp(lp + n1 - mix), np.exp(lp))
        Sv[:, :, j] = np.where(mj, np.abs(lp) + np.abs(n1) + np.abs(mix), np.abs(lp))
    n_obs = m.sum(-1)
    l, psi = np.logaddexp(A, B), np.repeat(np.exp(lpsi)[:, None], T, 1)
    q = np.exp(A - l)
    l, q = np.where(n_obs == 0, 0.0, l), np.where(n_obs == 0, psi, q)   # (what the formulas give there, stated exactly)
    cell = dict(A=A, B=B, l=l, q=q, psi=psi, n_obs=n_obs, S_A=SA, S_B=SB, S=SA + SB)
    out = {k: np.ascontiguousarray(v.T) for k, v in cell.items()}                                            # (N, T) -> (T, N)
    visit = dict(m=m, p=p, r=r, f_prob=q[:, :, None] * r, S_v=Sv)
    out.update({k: np.ascontiguousarray(v.transpose(2, 1, 0)) for k, v in visit.items()})                    # (N, T, J) -> (J, T, N)
    return out


def bounds(c, rtol):
    """(on log_lik (T, N), on z_prob (T, N), on f_prob (J, T, N)): see the module docstring."""
    bl, bq = L.bounds(c, rtol)
    _, bf = L.bounds(dict(S=c["S"], l=c["l"], A=c["A"], B=c["B"], S_B=c["S_B"], S_A=c["S_A"][None] + c["S_v"]), rtol)
    return bl, bq, bf


def brute_force_cell(psi, p, m, s, mu0, mu1, sg0, sg1):
    """One cell by enumeration of z and all 2^J values of f: (log_lik, P(z = 1 | data), [P(f_j = 1 | data)]); p, m, s are (J,)."""
    J = len(p)

    def norm(x, mu, sg):
        return np.exp(-0.5 * ((x - mu) / sg) ** 2) / (sg * np.sqrt(2 * np.pi))

    tot, tz, tf = 0.0, 0.0, np.zeros(J)
    for z in (0, 1):
        for f in itertools.product((0, 1), repeat=J):
            w = psi if z else 1.0 - psi
            for j in range(J):
                pf = z * p[j]
                w *= pf if f[j] else 1.0 - pf
                if m[j]:
                    w *= norm(s[j], mu1, sg1) if f[j] else norm(s[j], mu0, sg0)
            tot, tz, tf = tot + w, tz + z * w, tf + np.asarray(f) * w
    return np.log(tot), tz / tot, tf / tot


def frequency_case():
    """The inputs of the draw-frequency test (tests/test_gpu_scores.py): 850 sites x 2 periods x 10 visits with the simulator's own
    missingness, the simulator's true theta, and the number of times the draw is repeated -- 4000 draws of 68 kB of f_prob each, a
    little more than one 256 MB chunk of the entry's device scratch.  Returns X, W, scores (N, T, J), theta, n."""
    import contextlib
    import io

    from biolith_amd.models import simulate_cs

    with contextlib.redirect_stdout(io.StringIO()):
        data, truth = simulate_cs(n_sites=850, n_periods=2, deployment_days_per_site=70, simulate_missing=True, random_seed=2)
    th = np.r_[truth["beta"][0], truth["alpha"][0], 0.0, np.log(10.0), np.log(10.0), np.log(5.0)]
    return data["site_covs"], data["obs_covs"], data["obs"][0], th.astype(np.float32).astype(np.float64), 4000


def pooled_statistics(c, z_count, f_count, n, z_prob=None, f_prob=None, lo=0.05, hi=0.95):
    """Standardised sums of (z - z_prob) and of (f - f_prob) over the cells / visits whose probability lies in (lo, hi), for n joint
    draws at the theta of ``c`` (``cs_cells``' result); ``z_count`` (T, N) and ``f_count`` (J, T, N) count the ones among them,
    ``z_prob`` / ``f_prob`` are the probabilities the draws are held against (default: the restatement's own).  The z of different
    cells are independent Bernoulli(q).  The f of ONE cell are not: f_j = z b_j with b_j ~ Bernoulli(r_j) independent, so
    Cov(f_j, f_k) = q (1 - q) r_j r_k and the variance of a cell's sum is sum_j q r_j (1 - q r_j) + q (1 - q) ((sum_j r_j)^2 - sum_j r_j^2);
    a sum over the f standardised by sum p (1 - p) alone would be too wide by that term.  Returns {"z": (stat, count), "f": (stat, count)}."""
    q, r = c["q"], c["r"]
    zp, fp = (q if z_prob is None else np.asarray(z_prob, dtype=np.float64)), (c["f_prob"] if f_prob is None else np.asarray(f_prob, dtype=np.float64))
    mz = (q > lo) & (q < hi)
    stat_z = float((z_count[mz] - n * zp[mz]).sum() / np.sqrt(n * (q[mz] * (1 - q[mz])).sum()))
    mf = (c["f_prob"] > lo) & (c["f_prob"] < hi)
    rm, pm = np.where(mf, r, 0.0), np.where(mf, c["f_prob"], 0.0)
    var = (pm * (1 - pm)).sum(0) + q * (1 - q) * (rm.sum(0) ** 2 - (rm ** 2).sum(0))     # per cell
    stat_f = float((f_count[mf] - n * fp[mf]).sum() / np.sqrt(n * var.sum()))
    return {"z": (stat_z, int(mz.sum())), "f": (stat_f, int(mf.sum()))}
