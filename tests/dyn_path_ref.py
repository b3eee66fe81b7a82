"""Conditional dynamics of occu_dyn in float64 NumPy (TEST INFRASTRUCTURE): what ``bl_path_posterior`` returns, restated with the
terms, the clamp (a detection at z = 0 costs log(float32 tiny)) and the masks of the density the project already trusts
(oracle/occu_oracle.c: potential_grad_dyn; tests/test_dynamics_cpu.py pins this file to brute force over the 2^T paths and to that
oracle's potential).

``dyn_paths`` returns, per site (axis last): ``l`` (N,) the path-marginalised log-likelihood; ``q`` (T, N) = P(z_t = 1 | all seasons);
``col`` / ``ext`` (T - 1, N) = P(z_t = 0, z_t+1 = 1 | .) / P(z_t = 1, z_t+1 = 0 | .); the per-period terms ``a``, ``kb``, ``lpi``,
``l1m``, ``pi`` (the prior of season t given the seasons before it) and ``d`` (the filtered log-odds); ``n_obs`` (N,),
``n_obs_period`` (T, N); ``bk1`` / ``bk0`` (T - 1, N) = P(z_t = 1 | z_t+1 = 1 / 0, y_1..t), the backward kernels; ``psi``, ``gamma``, ``eps`` (N,); and ``S`` (N,), the sum over seasons of |visit terms| + |kb_t| + |log pi_t| +
|log(1 - pi_t)| -- the scale of a float32 evaluation's rounding error.

``dyn_paths_f32`` is the same recursion carried in ``np.float32`` the way the kernel carries it (complements as positive sums, pairs
normalised from the ratio of their parts): the CPU-side proof that the bounds below are reachable in that precision.
``parity_case`` builds the (data, theta) cases that the GPU parity test and the CPU emulation test share.
"""
import numpy as np

from latent_ref import ulp32

TINY = float(np.finfo(np.float32).tiny)


def _log_sigmoid(x):
    return -np.logaddexp(0.0, -x)


def _sigmoid(x):
    return np.exp(_log_sigmoid(x))


def _prepare(site_covs, obs_covs, obs):
    X, W, Y = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (site_covs, obs_covs, obs))
    if Y.ndim == 4:
        Y = Y[0]
    m = ~(np.isnan(Y) | np.isnan(W).any(-1) | np.isnan(X).any(-1)[:, None, None])          # (N, T, J)
    return np.nan_to_num(X), np.nan_to_num(W), np.nan_to_num(Y), m


def dyn_paths(site_covs, obs_covs, obs, th):
    """site_covs (N, Ks), obs_covs (N, T, J, Ko), obs (N, T, J) of the one species (NaN = missing), th = [b_psi | b_col | b_ext | alpha]."""
    X, W, Y, m = _prepare(site_covs, obs_covs, obs)
    th = np.asarray(th, dtype=np.float64)
    N, T, J, Ko = W.shape
    B = X.shape[1] + 1
    assert th.shape == (3 * B + Ko + 1,), th.shape
    eta = [th[b * B] + X @ th[b * B + 1:(b + 1) * B] for b in range(3)]
    al = th[3 * B:]
    psi, gam, ngam, eps, neps = _sigmoid(eta[0]), _sigmoid(eta[1]), _sigmoid(-eta[1]), _sigmoid(eta[2]), _sigmoid(-eta[2])
    nu = al[0] + W @ al[1:]
    det = Y != 0
    z1 = np.where(m, np.where(det, _log_sigmoid(nu), _log_sigmoid(-nu)), 0.0)
    z0 = np.where(m, np.where(det, np.log(TINY), np.log1p(-TINY)), 0.0)
    a, kb = z1.sum(-1).T, z0.sum(-1).T                                                     # (T, N)
    S = (np.abs(z1).sum(-1) + np.abs(z0).sum(-1)).T
    lpi, l1m, d, pi = (np.zeros((T, N)) for _ in range(4))
    l = np.zeros(N)
    lp, ln, p = _log_sigmoid(eta[0]), _log_sigmoid(-eta[0]), psi
    for t in range(T):
        lpi[t], l1m[t], pi[t] = lp, ln, p
        A, Bz = lp + a[t], ln + kb[t]
        l += np.logaddexp(A, Bz)
        d[t] = A - Bz
        f, g = _sigmoid(d[t]), _sigmoid(-d[t])
        p, n = f * neps + g * gam, f * eps + g * ngam
        lp, ln = np.log(p), np.log(n)
    S = (S + np.abs(lpi) + np.abs(l1m)).sum(0)
    q, col, ext, bk1, bk0 = np.zeros((T, N)), *(np.zeros((T - 1, N)) for _ in range(4))
    rho, nrho = _sigmoid(d[T - 1]), _sigmoid(-d[T - 1])
    q[T - 1] = rho
    for t in range(T - 2, -1, -1):
        f, g = _sigmoid(d[t]), _sigmoid(-d[t])
        p1, p0 = f * neps + g * gam, f * eps + g * ngam                                    # pi_t+1, 1 - pi_t+1
        x11, x01, x10, x00 = rho * f * neps / p1, rho * g * gam / p1, nrho * f * eps / p0, nrho * g * ngam / p0
        col[t], ext[t], bk1[t], bk0[t] = x01, x10, f * neps / p1, f * eps / p0
        rho, nrho = x11 + x10, x01 + x00
        q[t] = rho
    return dict(bk1=bk1, bk0=bk0, l=l, q=q, col=col, ext=ext, a=a, kb=kb, lpi=lpi, l1m=l1m, pi=pi, d=d, S=S, psi=psi, gamma=gam, eps=eps,
                n_obs=m.sum((1, 2)), n_obs_period=m.sum(-1).T)


def bounds(c, rtol):
    """The float32 kernel's allowance against this restatement: (on log_lik (N,), on z_prob / col_prob / ext_prob (N,), every season).
    log_lik: rtol times the sum of the absolute values of the site's terms plus half an ulp of the result.  Each probability is a
    sigmoid or a product of ratios of two path sums, each path sum carries at most the site's allowance, and |sigmoid'| <= 1/4: half
    of the site's allowance plus one ulp of 1."""
    bl = rtol * c["S"] + 0.5 * ulp32(c["l"])
    return bl, 0.5 * bl + 2.0 ** -23


def ffbs(c, rng, reps=1):
    """``reps`` joint draws (reps, T, N) of the path given the data from a ``dyn_paths`` result: forward filtering, backward sampling."""
    T, N = c["q"].shape
    z = np.zeros((reps, T, N), dtype=np.int8)
    z[:, T - 1] = rng.uniform(size=(reps, N)) < _sigmoid(c["d"][T - 1])
    for t in range(T - 2, -1, -1):
        z[:, t] = rng.uniform(size=(reps, N)) < np.where(z[:, t + 1] == 1, c["bk1"][t], c["bk0"][t])
    return z


def propagated_prior(psi, gamma, eps, T):
    """(..., T, N): P(z_t = 1 | theta) with no data at all, pi_1 = psi, pi_t+1 = pi_t (1 - eps) + (1 - pi_t) gamma; inputs (..., N)."""
    out = [np.asarray(psi, dtype=np.float64)]
    for _ in range(T - 1):
        out.append(out[-1] * (1.0 - eps) + (1.0 - out[-1]) * gamma)
    return np.stack(out, axis=-2)


def standardised(hit, prob, lo, hi):
    """(sum of hit - prob over the cells with lo < prob < hi) / sqrt(sum of prob (1 - prob)), and the number of those cells."""
    m = (prob > lo) & (prob < hi)
    pd = prob[m].astype(np.float64)
    return float((hit[m].astype(np.float64) - pd).sum() / np.sqrt((pd * (1 - pd)).sum())), int(m.sum())


def draws_case(N, T, J, seed):
    """(X, W, Y (1, N, T, J), centre): data simulated FROM the model at ``centre`` (psi ~ 0.5, gamma ~ eps ~ 0.15, detection ~ 0.27), so that
    many site-seasons stay ambiguous and neighbouring seasons are strongly dependent."""
    rng = np.random.default_rng(seed)
    X, W = rng.normal(size=(N, 1)), rng.normal(size=(N, T, J, 1))
    centre = np.array([0.0, 0.5, -1.7, 0.3, -1.7, -0.3, -1.0, 0.4])
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))  # noqa: E731
    psi, gam, eps = (sig(centre[2 * b] + centre[2 * b + 1] * X[:, 0]) for b in range(3))
    z = np.zeros((T, N))
    z[0] = rng.uniform(size=N) < psi
    for t in range(1, T):
        z[t] = rng.uniform(size=N) < np.where(z[t - 1] == 1, 1.0 - eps, gam)
    p = sig(centre[6] + centre[7] * W[..., 0])
    Y = ((rng.uniform(size=(N, T, J)) < p) & (z.T[:, :, None] == 1)).astype(np.float64)[None]
    return X, W, Y, centre


# ---- the kernel's arithmetic in float32 ----
_f = np.float32


def _sig32(x):
    e = np.exp(-np.abs(x))
    r = _f(1) / (_f(1) + e)
    return np.where(x > 0, _f(1), e) * r, np.where(x > 0, e, _f(1)) * r


def _lsig32(x):
    return np.minimum(x, _f(0)) - np.log1p(np.exp(-np.abs(x)))


def _norm32(a, b):
    hi, lo = np.maximum(a, b), np.minimum(a, b)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(hi > 0, lo / hi, _f(1)).astype(np.float32)
    r = _f(1) / (_f(1) + e)
    return np.where(a >= b, _f(1), e) * r, np.where(a >= b, e, _f(1)) * r


def dyn_paths_f32(site_covs, obs_covs, obs, th, positive_sums=True):
    """``l``, ``q``, ``col``, ``ext`` as ``dyn_paths`` gives them, every operation in float32.  ``positive_sums=False``: 1 - pi_t+1 by
    subtraction, the form that does not hold the bounds."""
    X, W, Y, m = (np.asarray(v) for v in _prepare(site_covs, obs_covs, obs))
    X, W = X.astype(np.float32), W.astype(np.float32)
    th = np.asarray(th, dtype=np.float32)
    N, T, J, Ko = W.shape
    B = X.shape[1] + 1
    eta = [(th[b * B] + X @ th[b * B + 1:(b + 1) * B]).astype(np.float32) for b in range(3)]
    al = th[3 * B:]
    (gam, ngam), (eps, neps) = _sig32(eta[1]), _sig32(eta[2])
    c = np.where(Y != 0, _f(1), _f(-1))
    v = np.where(m, _lsig32((c * (al[0] + W @ al[1:])).astype(np.float32)), _f(0)).astype(np.float32)
    nd = (m & (Y != 0)).sum(-1).T.astype(np.float32)
    nobs = m.sum(-1).T
    lp, ln = _lsig32(eta[0]), _lsig32(-eta[0])
    d = np.zeros((T, N), dtype=np.float32)
    l = np.zeros(N, dtype=np.float64)   # (the kernel's Kahan sum: the addends rounded to float32, their sum not)
    for t in range(T):
        A = (lp.astype(np.float64) + v[:, t].astype(np.float64).sum(-1)).astype(np.float32)   # (Kahan)
        Bz = (ln + nd[t] * _f(np.log(TINY))).astype(np.float32)
        d[t] = A - Bz
        norm = (np.maximum(A, Bz) + np.log1p(np.exp(-np.abs(d[t])))).astype(np.float32)
        l += np.where(nobs[t] > 0, norm, _f(0)).astype(np.float64)
        f, g = _sig32(d[t])
        p = (f * neps + g * gam).astype(np.float32)
        n = (f * eps + g * ngam).astype(np.float32) if positive_sums else (_f(1) - p).astype(np.float32)
        lp, ln = np.log(np.maximum(p, _f(TINY))), np.log(np.maximum(n, _f(TINY)))
    q, col, ext = (np.zeros((k, N), dtype=np.float32) for k in (T, max(T - 1, 0), max(T - 1, 0)))
    rho, nrho = _sig32(d[T - 1])
    q[T - 1] = rho
    for t in range(T - 2, -1, -1):
        f, g = _sig32(d[t])
        b1, nb1 = _norm32(f * neps, g * gam)
        b0, nb0 = _norm32(f * eps, g * ngam)
        col[t], ext[t] = rho * nb1, nrho * b0
        rho, nrho = _norm32(rho * b1 + ext[t], nrho * nb0 + col[t])
        q[t] = rho
    return dict(l=l.astype(np.float32), q=q, col=col, ext=ext)


# ---- the cases the GPU parity test and the CPU emulation test share ----
PARITY_T = (1, 2, 5, 16)
PARITY_K = ((0, 0), (2, 2), (8, 16))
PARITY_N = (70, 300)
RTOL = 1e-6   # the bound tests/test_gpu_dyn.py commits for this model's bl_logp_grad
E2E = dict(n_sites=300, n_periods=5, random_seed=1)   # simulate_dyn's arguments for the end-to-end tests, on the CPU and on the device


def parity_case(T, Ks, Ko, N, J=4):
    """(X, W, Y (1, N, T, J), th (4, D)): the missing-data pattern of test_gpu_latent._occu_arrays (30 % of the visits, four whole
    sites, a site covariate, an obs covariate), one season fully unobserved for 30 sites when T > 2; theta ~ U(-2, 2), times 0.35 with
    16 covariates on a side, the last row pushed out as test_gpu_dyn.py does (psi ~ 1, gamma ~ eps ~ 1e-3)."""
    rng = np.random.default_rng(1000 * T + 10 * Ks + Ko + N)
    X, W = rng.normal(size=(N, Ks)), rng.normal(size=(N, T, J, Ko))
    Y = (rng.uniform(size=(1, N, T, J)) < 0.3).astype(np.float64)
    Y[rng.uniform(size=Y.shape) < 0.3] = np.nan
    Y[0, :4] = np.nan
    if Ks:
        X[6, 0] = np.nan
    if Ko:
        W[8, 0, 1, 0] = np.nan
    if T > 2:
        Y[0, 20:50, 1] = np.nan
    D = 3 * (Ks + 1) + Ko + 1
    th = rng.uniform(-2, 2, size=(4, D)) * (0.35 if max(Ks, Ko) > 8 else 1.0)
    th[3, [0, Ks + 1, 2 * (Ks + 1)]] = [6.0, -7.0, -7.0]
    return X, W, Y, th.astype(np.float32).astype(np.float64)
