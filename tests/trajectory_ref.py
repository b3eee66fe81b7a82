"""The definition of ``trajectory_totals`` in NumPy float64 (TEST INFRASTRUCTURE), written from the model's statement and independent
of the library: per posterior draw and site of ``occu_dyn``

    psi, gamma, eps = logistic(b . (1, x)) for beta, beta_col, beta_ext       (float32 covariates, NaN -> 0, and coefficients, promoted)
    pi_1 = psi,    pi_t+1 = pi_t (1 - eps) + (1 - pi_t) gamma
    colonised_t = (1 - pi_t) gamma,   extinct_t = pi_t eps,   equilibrium = gamma / (gamma + eps)
    the path: cell (n, t, i) takes one uniform u of bl_cell_rng(seed, n, T, t, N, i) (tests/pred_rng_ref.py);
              z_1 = u < psi,   z_t+1 = u < (z_t ? 1 - eps : gamma)

and per region the float64 sum of ``w_i`` times the term.  ``brute_force`` enumerates the 2^T paths of one site instead.

THE BOUND.  It is derived, not measured; u = 2^-53, everything to first order, periods t = 0 .. T-1.

*A rate.*  The kernel forms eta as an fma chain of Ks steps, each rounding at most u |partial| <= u A, A = |b_0| + sum_k |x_k b_k| (the
products are exact: two float32 values); NumPy's dot and one addition round Ks times too: eta is off by at most Ks A u, a logistic by
a quarter of that (its slope).  The kernel's sigmoid is e = exp(-|eta|) (1 ulp = 2u relative), r = 1 / (1 + e), s = e r: r carries
e / (1 + e) 2u <= u of the exponential's error and two roundings, 3u relative and absolute (r <= 1); s carries 2u + 3u + u = 6u relative,
s <= 1/2: 3u absolute.  NumPy's 1 / (1 + exp(-eta)) carries 2u + u + u = 4u relative at the worst, and this side forms a complement as
1 - x, one rounding more (the kernel takes it from the sigmoid, sigma(-eta)).  With A_i the largest A of the three predictors, every
rate and every complement of one, on either side, is off by at most

    r_i = (5 + Ks A_i / 4) u                                                   [the issue's: 4u + Ks A u / 4, and u for this side's 1 - x]

*A step.*  The kernel carries the pair (pi, q): col = fl(q gamma), ext = fl(pi eps), pi' = fma(pi, 1 - eps, col), q' = fma(q, 1 - gamma, ext).
With d. the error of a computed value:  |d pi'| <= |d pi| (1 - eps) + |d q| gamma + (pi + q) r + u q gamma + u pi'  and the same for q'
with eps, 1 - gamma.  The two columns (1 - eps, eps) and (gamma, 1 - gamma) each sum to 1, so S = |d pi| + |d q| is not amplified:
S' <= S + 2r + 2u (pi' + q' = 1, q gamma <= pi', pi eps <= q').  S_0 <= 2r, so

    |d pi_t| <= S_t <= (t + 1)(2r + 2u) = (t + 1)(12 + Ks A_i / 2) u           [the issue's: (t + 1)(12 + Ks A_i) u: this one is not larger]

This side forms q as fl(1 - pi), d q = -d pi + u, so d pi' = d pi ((1 - eps) - gamma) + .., |(1 - eps) - gamma| <= 1, five roundings
and two rates: |d pi_t| <= r + t (r + 4u), below the same bound since r >= 2u.

*The pair terms.*  col_t = fl(q_t gamma): |d q_t| + r + u <= S_t + r + u; here (|d pi_t| + u) + r + u.  Both are below
(t + 2)(2r + 2u): ``t + 2`` in place of ``t + 1``, as the issue has it.

*The equilibrium.*  v = gamma / fl(gamma + eps): d v = (d gamma eps - gamma d eps) / (gamma + eps)^2, at most r / (gamma + eps), and two
roundings of v <= 1:  r / (gamma + eps) + 2u                                   [the issue's: (4u + 2r) / (gamma + eps), LARGER]

*A weighted term and a total.*  Each side rounds the product w_i v_i once.  Two sides differ per term by at most
2 |w_i| bound_i + 2u |w_i v_i|; the sum over a region adds 2 (N_g - 1) u sum |w_i v_i|, as in tests/totals_ref.py.  ``check`` asserts
that the whole stays below 1e-12 sum |w_i| for the shapes it is handed (N <= 300, T <= 8, coefficients in (-1, 1): about 1e-13), so
no comparison is vacuous.

*The path.*  Both sides compare the same uniform, a multiple of 2^-24, with their own threshold; the thresholds are within 2r + 2u of
each other.  A cell whose uniform lies within that of this side's threshold may legitimately come out differently; ``path`` counts
such cells along its own path (by induction the two paths agree up to the first one) and every test asserts the count is 0, so the
realised totals are EQUAL to this restatement: ``ordered_sum`` adds the products w_i z_i in the device's order -- the region's sites
in site order in runs of 64, the last filled up with -0.0, a run as the tree (x_l + x_{l+32}), then 16, 8, 4, 2, 1 apart, the runs in
order -- so the equality holds for any weights, not for unit weights alone."""
import itertools

import numpy as np

import pred_rng_ref
from totals_ref import region_sites

U = 2.0 ** -53
EXPECTED = ("occupancy", "colonised", "extinct", "equilibrium")
REALISED = ("z", "z_colonised", "z_extinct")
BLOCKS = ("beta", "beta_col", "beta_ext")


def rates(site_covs, sites):
    """-> (psi, gamma, eps) each (n, N) float64, and RATE (n, N): the bound on a rate or on its complement, (5 + Ks A / 4) u."""
    X = np.nan_to_num(np.asarray(site_covs, dtype=np.float32)).astype(np.float64)            # (N, Ks)
    out, A = [], 0.0
    for name in BLOCKS:
        b = np.asarray(sites[name], dtype=np.float32)[:, 0, :].astype(np.float64)            # (n, Ks + 1)
        assert b.shape[1] == X.shape[1] + 1
        eta = b[:, :1] + b[:, 1:] @ X.T
        out.append(1.0 / (1.0 + np.exp(-eta)))
        A = np.maximum(A, np.abs(b[:, :1]) + np.abs(b[:, 1:]) @ np.abs(X.T))
    return out[0], out[1], out[2], (5.0 + X.shape[1] * A / 4.0) * U


def expected(site_covs, sites, T):
    """The expected terms per (draw, site) and the bound on each: two dicts under ``EXPECTED``; ``occupancy`` (n, T, N),
    ``colonised`` / ``extinct`` (n, T - 1, N), ``equilibrium`` (n, N)."""
    psi, gam, eps, r = rates(site_covs, sites)
    n, N = psi.shape
    occ, col, ext = np.empty((n, T, N)), np.empty((n, max(T - 1, 0), N)), np.empty((n, max(T - 1, 0), N))
    pi = psi
    for t in range(T):
        occ[:, t] = pi
        if t + 1 < T:
            col[:, t], ext[:, t] = (1.0 - pi) * gam, pi * eps
            pi = pi * (1.0 - eps) + (1.0 - pi) * gam
    step = 2.0 * r + 2.0 * U
    values = dict(occupancy=occ, colonised=col, extinct=ext, equilibrium=gam / (gam + eps))
    bounds = dict(occupancy=np.stack([(t + 1) * step for t in range(T)], axis=1),
                  colonised=np.stack([(t + 2) * step for t in range(T - 1)], axis=1) if T > 1 else np.empty((n, 0, N)),
                  equilibrium=r / (gam + eps) + 2.0 * U)
    bounds["extinct"] = bounds["colonised"]
    return values, bounds


def path(site_covs, sites, T, seed, first_draw=0, of=None):
    """One ancestral path per draw by the device's generator: ``z`` (n, T, N) bool, and the number of cells whose uniform lies within
    the two sides' threshold difference of the threshold (0: the device's path must equal this one).  ``of = (index, N_all)``: the
    rows of ``site_covs`` are the sites ``index`` of a handle of ``N_all`` sites (a cell is keyed by the site's own index)."""
    psi, gam, eps, r = rates(site_covs, sites)
    n, N = psi.shape
    index, N_all = (None, N) if of is None else of
    u = pred_rng_ref.cells(seed, first_draw + np.arange(n), T, N_all, index).uniform()       # (n, T, N)
    z, near = np.empty((n, T, N), dtype=bool), 0
    for t in range(T):
        thr = psi if t == 0 else np.where(z[:, t - 1], 1.0 - eps, gam)
        z[:, t] = u[:, t] < thr
        near += int(np.count_nonzero(np.abs(u[:, t] - thr) <= 2.0 * r + 2.0 * U))
    return z, near


def realised(z):
    """The path's terms under ``REALISED``: ``z`` (n, T, N), ``z_colonised`` / ``z_extinct`` (n, T - 1, N), float64 zeros and ones."""
    return dict(z=z.astype(np.float64), z_colonised=(~z[:, :-1] & z[:, 1:]).astype(np.float64),
                z_extinct=(z[:, :-1] & ~z[:, 1:]).astype(np.float64))


def brute_force(psi, gam, eps, T):
    """One site by enumeration of its 2^T paths: (pi (T,), colonised (T - 1,), extinct (T - 1,)), the sums of the paths' probabilities."""
    pi, col, ext = np.zeros(T), np.zeros(max(T - 1, 0)), np.zeros(max(T - 1, 0))
    for zs in itertools.product((0, 1), repeat=T):
        pr = psi if zs[0] else 1.0 - psi
        for a, b in zip(zs[:-1], zs[1:]):
            pr *= ((1.0 - eps) if b else eps) if a else (gam if b else 1.0 - gam)
        for t in range(T):
            pi[t] += pr * zs[t]
        for t in range(T - 1):
            col[t] += pr * (zs[t] == 0 and zs[t + 1] == 1)
            ext[t] += pr * (zs[t] == 1 and zs[t + 1] == 0)
    return pi, col, ext


def ratio(num, den):
    """``num / den``, NaN where ``den`` is zero."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den == 0, np.nan, num / den)


def growth_rate(occupancy):
    """(n, T, ...) -> (n, T - 1, ...): occupancy[t + 1] / occupancy[t]."""
    return ratio(occupancy[:, 1:], occupancy[:, :-1])


def turnover(colonised, occupancy):
    """(n, T - 1, ...), (n, T, ...) -> (n, T - 1, ...): colonised[t] / occupancy[t + 1], the share of a season's occupied area that is new."""
    return ratio(colonised, occupancy[:, 1:])


def ordered_sum(terms):
    """(..., N_g) -> (...): the device's sum of a region's terms, bit for bit (the module docstring)."""
    terms = np.asarray(terms, dtype=np.float64)
    runs = -(-terms.shape[-1] // 64)
    a = np.full(terms.shape[:-1] + (runs * 64,), -0.0)
    a[..., :terms.shape[-1]] = terms
    a = a.reshape(terms.shape[:-1] + (runs, 64))
    for o in (32, 16, 8, 4, 2, 1):
        a = a[..., :o] + a[..., o:2 * o]
    total = a[..., 0, 0] if runs else np.zeros(terms.shape[:-1])
    for k in range(1, runs):
        total = total + a[..., k, 0]
    return total


def check_summaries(entry, probs, label=""):
    """mean, sd (ddof 1, NaN for one draw) and quantiles (linear) are NumPy's on ``draws``, NaNs where NumPy has them."""
    d = entry["draws"]
    assert set(entry) == {"draws", "mean", "sd", "quantiles"} and d.dtype == np.float64, label
    same = lambda a, b: np.array_equal(a, b, equal_nan=True)
    assert same(entry["mean"], np.mean(d, axis=0)), label
    if d.shape[0] > 1:
        assert same(entry["sd"], np.std(d, axis=0, ddof=1)), label
    else:
        assert entry["sd"].shape == d.shape[1:] and np.isnan(entry["sd"]).all(), label
    assert same(entry["quantiles"], np.quantile(d, np.asarray(probs, dtype=np.float64), axis=0)), label
    assert entry["quantiles"].shape == (len(probs),) + d.shape[1:], label


def check_terms(res, site_covs, sites, T, weights, seed, of=None):
    """The engine's arrays where every site is its own region -- ``res[name][..., j]`` is site j's term, ``w_j`` times its value --
    against the definition: the expected terms within the per-term bound, the realised ones equal.  ``of`` as in ``path``."""
    w = np.asarray(weights, dtype=np.float64)
    values, bounds = expected(site_covs, sites, T)
    for name in EXPECTED:
        want = w * values[name]
        bound = 2.0 * np.abs(w) * bounds[name] + 2.0 * U * np.abs(want)
        assert np.all(bound <= 1e-12 * np.abs(w)), (name, float(bound.max()))                # not vacuous
        assert np.all(np.abs(res[name] - want) <= bound), (name, float(np.abs(res[name] - want).max()), float(bound.max()))
    z, near = path(site_covs, sites, T, seed, of=of)
    assert near == 0, ("cells at a threshold", near)
    for name, terms in realised(z).items():
        assert np.array_equal(res[name], w * terms), name


def check(got, site_covs, sites, T, regions=None, weights=None, probs=(0.05, 0.5, 0.95), seed=0, latent=True, label=""):
    """The wrapper's result against the definition.  Returns the largest error of an expected total as a fraction of its bound."""
    N = np.shape(site_covs)[0]
    n = np.asarray(sites["beta"]).shape[0]
    labels, idxs = region_sites(regions, N)
    G = len(idxs)
    w = np.ones(N) if weights is None else np.asarray(weights, dtype=np.float64)
    assert np.array_equal(got["regions"], labels), label
    assert np.array_equal(got["n_sites"], [len(idx) for idx in idxs]) and got["n_sites"].dtype.kind == "i", label
    for g, idx in enumerate(idxs):
        assert abs(got["weight"][g] - w[idx].sum()) <= 2.0 * max(len(idx) - 1, 0) * U * np.abs(w[idx]).sum(), (label, g)
    assert got["n_draws"] == n and got["n_periods"] == T and np.array_equal(got["probs"], np.asarray(probs, dtype=np.float64)), label
    names = EXPECTED + ("growth_rate", "turnover") + (REALISED if latent else ())
    assert set(got) == {"regions", "n_sites", "weight", "probs", "n_draws", "n_periods"} | set(names), (label, sorted(got))
    shape = lambda name: (n, G, 1) if name == "equilibrium" else (n, T if name in ("occupancy", "z") else T - 1, G, 1)
    for name in names:
        d = got[name]["draws"]
        assert d.shape == shape(name) and d.dtype == np.float64, (label, name, d.shape)
        check_summaries(got[name], probs, f"{label} {name}")

    values, bounds = expected(site_covs, sites, T)
    worst = 0.0
    for name in EXPECTED:
        d = got[name]["draws"][..., 0]
        for g, idx in enumerate(idxs):
            terms = w[idx] * values[name][..., idx]
            want, mass = np.sum(terms, axis=-1), np.sum(np.abs(terms), axis=-1)
            bound = 2.0 * np.sum(np.abs(w[idx]) * bounds[name][..., idx], axis=-1) + 2.0 * U * mass + 2.0 * max(len(idx) - 1, 0) * U * mass
            assert np.all(bound <= 1e-12 * np.abs(w[idx]).sum()), (label, name, g, float(bound.max()))   # not vacuous
            err = np.abs(d[..., g] - want)
            assert np.isfinite(d[..., g]).all() and np.all(err <= bound), (label, name, g, float(err.max()), float(bound.max()))
            worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0)))
    # formed on the host from the draws
    occ, col = got["occupancy"]["draws"], got["colonised"]["draws"]
    assert np.array_equal(got["growth_rate"]["draws"], growth_rate(occ), equal_nan=True), label
    assert np.array_equal(got["turnover"]["draws"], turnover(col, occ), equal_nan=True), label
    if latent:
        z, near = path(site_covs, sites, T, seed)
        assert near == 0, (label, "cells at a threshold", near)
        for name, terms in realised(z).items():
            d = got[name]["draws"][..., 0]
            for g, idx in enumerate(idxs):
                assert np.array_equal(d[..., g], ordered_sum(w[idx] * terms[..., idx])), (label, name, g)
    return worst
