"""Conditional occupancy in float64 NumPy (TEST INFRASTRUCTURE): per (period, site) cell the two branches of the z-marginalised
likelihood, A = log psi + log p(obs | z = 1) and B = log(1 - psi) + log p(obs | z = 0), l = logaddexp(A, B), q = exp(A - l), for
every family ``bl_site_posterior`` serves, with the clamps and masks of the densities the project already trusts:

occu (plain, false positives, random effects) -- the oracle's statement (oracle/occu_oracle.c; tests/test_reference_logjoint.py pins
    it to the reference's own model to 1e-10 outside the clamp regime): exact logs in the z = 1 branch and for psi; a detection at
    z = 0 without a false-positive rate costs log(float32 tiny), a non-detection log1p(-tiny); with a rate f the z = 0 branch is
    Bernoulli(f).  A visit is masked where y, one of its covariates or a site covariate is NaN.
occu_comb -- tests/comb_ref.py cell by cell: every Bernoulli probability clipped to [tiny, 1 - eps].

Each function returns a dict of (T, N) float64 arrays: A, B, l, q, psi, n_obs, and S_A / S_B, the sums of the absolute values of the
terms of each branch (the scale of a float32 evaluation's rounding error; S = S_A + S_B).
"""
import numpy as np

TINY, EPS = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).eps)


def _log_sigmoid(x):
    return -np.logaddexp(0.0, -x)


def _finish(A, B, SA, SB, psi, n_obs):
    l = np.logaddexp(A, B)
    out = dict(A=A, B=B, l=l, q=np.exp(A - l), psi=np.broadcast_to(psi[:, None], A.shape), n_obs=n_obs, S_A=SA, S_B=SB, S=SA + SB)
    return {k: np.ascontiguousarray(np.asarray(v).T) for k, v in out.items()}   # (N, T) -> (T, N)


def occu_theta_layout(N, T, J, Ks, Ko, fp=False, site_re=False, obs_re=False):
    """Offsets of the engine's one-species coordinates: [beta, alpha, (phi), (log site sd), (log obs sd), u [N], v [N], e [N][T][J]]."""
    at = Ks + Ko + 2
    o = dict(fp=-1, u=-1, v=-1, e=-1)
    if fp:
        o["fp"] = at
        at += 1
    at += int(site_re) + int(obs_re)
    if site_re:
        o["u"], o["v"] = at, at + N
        at += 2 * N
    if obs_re:
        o["e"] = at
        at += N * T * J
    o["D"] = at
    return o


def occu_cells(site_covs, obs_covs, obs, th, fp_mode=None, site_re=False, obs_re=False):
    """site_covs (N, Ks), obs_covs (N, T, J, Ko), obs (N, T, J) of ONE species (NaN = missing), th the engine's flat coordinates."""
    X, W, Y = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (site_covs, obs_covs, obs))
    th = np.asarray(th, dtype=np.float64)
    N, T, J, Ko = W.shape
    Ks = X.shape[1]
    o = occu_theta_layout(N, T, J, Ks, Ko, fp_mode is not None, site_re, obs_re)
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
    lpsi, l1psi = _log_sigmoid(eta), _log_sigmoid(-eta)
    det = Y > 0
    if fp_mode is None:
        z1 = np.where(det, _log_sigmoid(nu), _log_sigmoid(-nu))
        z0 = np.where(det, np.log(TINY), np.log1p(-TINY))
    else:
        phi = th[o["fp"]]
        lf, l1f = _log_sigmoid(phi), _log_sigmoid(-phi)
        z0 = np.where(det, lf, l1f)
        if fp_mode == "constant":   # P(y = 1 | z = 1) = p + f (1 - p), P(y = 0 | z = 1) = (1 - p)(1 - f)
            z1 = np.where(det, np.logaddexp(_log_sigmoid(nu), lf + _log_sigmoid(-nu)), _log_sigmoid(-nu) + l1f)
        else:
            assert fp_mode == "unoccupied"
            z1 = np.where(det, _log_sigmoid(nu), _log_sigmoid(-nu))
    z1, z0 = np.where(m, z1, 0.0), np.where(m, z0, 0.0)
    A, B = lpsi[:, None] + z1.sum(-1), l1psi[:, None] + z0.sum(-1)
    SA, SB = np.abs(lpsi)[:, None] + np.abs(z1).sum(-1), np.abs(l1psi)[:, None] + np.abs(z0).sum(-1)
    return _finish(A, B, SA, SB, np.exp(lpsi), m.sum(-1))


def _log_bern(y, p):
    p = np.clip(p, TINY, 1.0 - EPS)
    return np.where(y > 0, np.log(p), np.log1p(-p))


def _log_norm(x, loc, scale):
    return -0.5 * ((x - loc) / scale) ** 2 - np.log(scale) - 0.5 * np.log(2 * np.pi)


def comb_cells(ref, th):
    """``ref``: a tests/comb_ref.py ``CombRef`` (its data, masks and clamps); th = [beta | alpha_PC | alpha_ARU | logit fc | logit fu | mu0 |
    log(mu1 - mu0) | log sigma0 | log sigma1]."""
    beta, apc, aar, e = ref.split(np.asarray(th, dtype=np.float64))
    fc, fu = 1 / (1 + np.exp(-e[0])), 1 / (1 + np.exp(-e[1]))
    mu0, mu1, s0, s1 = e[2], e[2] + np.exp(e[3]), np.exp(e[4]), np.exp(e[5])
    psi = 1 / (1 + np.exp(-(beta[0] + ref.X @ beta[1:])))
    p_pc = 1 / (1 + np.exp(-(apc[0] + ref.Wp @ apc[1:])))
    p_ar = 1 / (1 + np.exp(-(aar[0] + ref.Wa @ aar[1:])))
    branch, scale = [], []
    for z in (0, 1):
        lz = _log_bern(np.full(psi.shape, float(z)), psi)[:, None]
        p_fp = 1 - (1 - z * p_ar) * (1 - fc) * (1 - (1 - z) * fu)
        terms = [np.where(ref.mp, _log_bern(ref.Yp, z * p_pc), 0.0), np.where(ref.ma, _log_bern(ref.Ya, p_fp), 0.0),
                 np.where(ref.ms, _log_norm(ref.Sc, mu1 if z else mu0, s1 if z else s0), 0.0)]
        branch.append(lz + sum(t.sum(-1) for t in terms))
        scale.append(np.abs(lz) + sum(np.abs(t).sum(-1) for t in terms))
    n_obs = ref.mp.sum(-1) + ref.ma.sum(-1) + ref.ms.sum(-1)
    return _finish(branch[1], branch[0], scale[1], scale[0], np.clip(psi, TINY, 1.0 - EPS), n_obs)


def ulp32(x):
    """Spacing of float32 at |x| (float64 array)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def bounds(c, rtol):
    """The float32 kernel's allowance per cell against this restatement: (on log_lik, on z_prob).  log_lik: rtol times the sum of
    the absolute values of the cell's terms plus half an ulp of the result; z_prob = sigmoid(A - B) with |sigmoid'| <= 1/4: a quarter
    of the allowances of A and B plus one ulp of 1."""
    bl = rtol * c["S"] + 0.5 * ulp32(c["l"])
    bA, bB = rtol * c["S_A"] + 0.5 * ulp32(c["A"]), rtol * c["S_B"] + 0.5 * ulp32(c["B"])
    return bl, 0.25 * (bA + bB) + 2.0 ** -23
