"""PSIS-LOO of one cell in float64 NumPy (TEST INFRASTRUCTURE): the restatement of the definition that ``bl_psis_loo``
(include/biolith_hip.h) implements, one column of the (draws, cells) log-likelihood matrix at a time.  BUILDER-DEFINED: the reference
has no leave-one-out criterion; the definition is Vehtari, Simpson, Gelman, Yao and Gabry's Pareto-smoothed importance sampling with
r_eff = 1 and Zhang and Stephens' profile posterior mean for the generalised-Pareto fit (with the weakly informative prior on k).

For a column ``ll[0..n-1]`` (float32 widened exactly, all finite, n >= 2):

    lr = -ll - max(-ll)                                  the log ratios, the largest exactly 0
    M = ceil(min(n / 5, 3 sqrt(n)))                      cut = max((M+1)-th largest lr, LOG_DBL_MIN)   (n < 5: the smallest lr)
    tail = {s: lr_s > cut}, M' of them; M' <= 4: k = inf and lr stays; otherwise the tail is fitted and its lr replaced by the
    fit's expected order statistics, capped at 0
    lw = lr - logsumexp(lr);  elpd = logsumexp(lw + ll);  lppd = logsumexp(ll) - log n

``column(ll)`` returns ``(elpd, k, lppd)``; ``matrix(ll)`` the three (cells,) arrays of an (n, cells) matrix, NaN for a column that holds
a non-finite value.
"""
import numpy as np

LOG_DBL_MIN = -708.3964185322641   # log(DBL_MIN) as float64: written out, so that no two logarithm routines can disagree on it
EPS = float(np.finfo(np.float64).eps)


def tail_length(n):
    """M of the definition."""
    return int(np.ceil(min(n / 5.0, 3.0 * np.sqrt(float(n)))))


def _logsumexp(a):
    m = np.max(a)
    return m + np.log(np.sum(np.exp(a - m)))


def gpd_fit(x):
    """(k, sigma) of the ascending, positive exceedances x: Zhang and Stephens' profile posterior mean, prior of weight 10 at 0.5."""
    Mp = len(x)
    m = 30 + int(np.floor(np.sqrt(float(Mp))))
    j = np.arange(1, m + 1, dtype=np.float64)
    xq = x[int(np.floor(Mp / 4.0 + 0.5)) - 1]
    with np.errstate(all="ignore"):
        b = (1.0 - np.sqrt(m / (j - 0.5))) / (3.0 * xq) + 1.0 / x[-1]
        kk = np.array([np.mean(np.log1p(-bj * x)) for bj in b])
        L = Mp * (np.log(-b / kk) - kk - 1.0)
        w = np.array([1.0 / np.sum(np.exp(L - Lj)) for Lj in L])
        keep = ~(w < 10.0 * EPS)
        w = np.where(keep, w, 0.0)
        w = w / np.sum(w)
        bb = float(np.sum(w * b))
        k0 = float(np.mean(np.log1p(-bb * x)))
        sigma = -k0 / bb
    return (Mp * k0 + 5.0) / (Mp + 10.0), sigma


def smoothed_log_ratios(ll):
    """(lr after smoothing, k) of one column."""
    ll = np.asarray(ll, dtype=np.float64)
    n = ll.shape[0]
    assert ll.ndim == 1 and n >= 2 and np.all(np.isfinite(ll))
    neg = -ll
    lr = neg - np.max(neg)
    M = tail_length(n)
    desc = np.sort(lr)[::-1]
    cut = max(desc[M] if M + 1 <= n else desc[-1], LOG_DBL_MIN)
    tail = np.nonzero(lr > cut)[0]
    Mp = len(tail)
    if Mp <= 4:
        return lr, np.inf
    order = tail[np.argsort(lr[tail], kind="stable")]
    ecut = np.exp(cut)
    x = np.exp(lr[order]) - ecut
    k, sigma = gpd_fit(x)
    if np.isfinite(k):
        p = (np.arange(Mp) + 0.5) / Mp
        with np.errstate(all="ignore"):
            q = -np.log1p(-p) if abs(k) < 1e-15 else np.expm1(-k * np.log1p(-p)) / k
            v = np.log(sigma * q + ecut)
        lr = lr.copy()
        lr[order] = np.where(v > 0.0, 0.0, v)
    return lr, float(k)


def column(ll):
    """(elpd_i, k_i, lppd_i) of one column."""
    ll = np.asarray(ll, dtype=np.float64)
    lr, k = smoothed_log_ratios(ll)
    lw = lr - _logsumexp(lr)
    return float(_logsumexp(lw + ll)), k, float(_logsumexp(ll) - np.log(float(ll.shape[0])))


def matrix(ll):
    """Three (cells,) float64 arrays of an (n, cells) matrix; a column that holds a non-finite value is NaN in all three."""
    ll = np.asarray(ll)
    out = np.full((3, ll.shape[1]), np.nan)
    for c in range(ll.shape[1]):
        col = ll[:, c].astype(np.float64)
        if np.all(np.isfinite(col)):
            out[:, c] = column(col)
    return out[0], out[1], out[2]
