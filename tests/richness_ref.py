"""The definition of ``species_richness`` in NumPy, on ``predict()``'s float32 ``psi``: the Poisson-binomial recursion over the species,
the site sums over the draws in draw order, the area sums in the device's order, and the bounds within which a second float64
evaluation agrees.  The bounds are derived, not measured; ``u = 2^-53``.

Recursion.  ``p = (double) psi_s`` is exact, ``q = 1 - p`` one rounding, and a step ``pi[r] q + pi[r - 1] p`` two products and a sum:
four roundings a step, every term non-negative, so nothing cancels and the error is RELATIVE: after S species an entry is within
``4 S u`` of the exact pmf (first order; float64 NumPy stayed within ``1.0 S u`` of exact rational arithmetic for S <= 32 on random
psi, exact 0 and 1 included).  Two float64 evaluations of it -- this file's and the device's, which may round a step otherwise --
therefore differ by at most ``8 S u pi`` per entry.

The bound is relative, so it holds only while nothing underflows: ``assert_scaled`` asserts that every non-zero entry is above
``2^-900``.  (An entry that is exactly zero came from a factor that is exactly zero -- a float32 psi of 0 or 1 --, is zero in every
evaluation, and is within any relative bound.)  Coefficients in (-1, 1) on standard-normal covariates with S <= 32 keep to that.

Site sums.  A sum of n non-negative terms in any order is within ``(n - 1) u`` of exact, relative; two of them: ``2 (n - 1) u``.  So
``pmf`` is compared at ``(8 S + 2 (n - 1)) u pmf``.  ``E = sum_s p`` runs over exact float64 values; it is compared, like its mean over
the draws, at ``(2 (S - 1) + 2 (n - 1)) u``.  The sd of E is two-pass: with ``dm`` the two means' difference, every ``d = E - mean``
moves by at most ``dm``, which moves ``sqrt(M2 / (n - 1))`` by at most ``sqrt(n / (n - 1)) dm <= 2 dm`` (Cauchy-Schwarz), and the
roundings of d, d^2, the sum, the division and the root are ``(n + 4) u / 2`` relative an evaluation:
``|sd - sd'| <= (n + 4) u sd + 2 dm_max``, ``dm_max`` the bound of the mean.

Area sums.  ``sum_{i in g} w_i pi_i``: the terms differ by ``8 S u |w_i| pi_i``, and two sums of the same N_g terms by ``regional_totals``'
``2 (N_g - 1) u sum |w_i pi_i|`` (tests/totals_ref.py): ``(8 S + 2 (N_g - 1)) u sum_i |w_i| pi_i``.  The sum below is in the device's
order all the same -- runs of 64 sites, the tree over lanes 32, 16, .. 1 apart with -0.0 in the idle lanes, the runs in order."""
import numpy as np

U = 2.0 ** -53
FLOOR = 2.0 ** -900


def pmf(psi32):
    """``psi32`` (..., S) float32 -> (pi (..., S + 1), E (...)) float64: the recursion over the species in ascending order."""
    psi32 = np.asarray(psi32)
    assert psi32.dtype == np.float32
    S = psi32.shape[-1]
    pi = np.zeros(psi32.shape[:-1] + (S + 1,))
    pi[..., 0] = 1.0
    E = np.zeros(psi32.shape[:-1])
    for s in range(S):
        p = psi32[..., s].astype(np.float64)
        q = 1.0 - p
        E = E + p
        shifted = np.concatenate([np.zeros(pi.shape[:-1] + (1,)), pi[..., :-1]], axis=-1)   # pi[r - 1], pi[-1] = 0
        stay, come = pi * q[..., None], shifted * p[..., None]
        pi = stay + come
    return pi, E


def assert_scaled(pi):
    """The relative bounds hold: no entry has come near underflow."""
    positive = pi[pi != 0.0]
    assert positive.size and positive.min() > FLOOR, float(positive.min(initial=1.0))
    assert np.all(pi >= 0.0)


def site_outputs(psi32):
    """``psi32`` (n, N, S) -> (pmf (N, S + 1), expected_mean (N,), expected_sd (N,)): one accumulator per entry in ascending draw order,
    the sd by a second pass (NaN for one draw)."""
    pi, E = pmf(psi32)
    assert_scaled(pi)
    n = pi.shape[0]
    acc, esum = np.zeros(pi.shape[1:]), np.zeros(E.shape[1:])
    for k in range(n):
        acc, esum = acc + pi[k], esum + E[k]
    mean = esum / n
    m2 = np.zeros_like(mean)
    for k in range(n):
        d = E[k] - mean
        m2 = m2 + d * d
    with np.errstate(invalid="ignore", divide="ignore"):
        sd = np.sqrt(m2 / (n - 1)) if n > 1 else np.full(mean.shape, np.nan)
    return acc / n, mean, sd


def site_bounds(psi32, pmf_mean, e_mean, e_sd):
    """The bounds of (pmf, expected_mean, expected_sd) for a second evaluation."""
    n, _, S = psi32.shape
    b_mean = (2.0 * (S - 1) + 2.0 * (n - 1)) * U * e_mean
    b_sd = (n + 4) * U * e_sd + 2.0 * b_mean if n > 1 else np.zeros_like(e_mean)
    return (8.0 * S + 2.0 * (n - 1)) * U * pmf_mean, b_mean, b_sd


def wave_tree(x):
    """``x`` (..., 64) -> (...): the tree over lanes 32, 16, .. 1 apart."""
    assert x.shape[-1] == 64
    o = 32
    while o:
        x = x[..., :o] + x[..., o:2 * o]
        o //= 2
    return x[..., 0]


def area(pi, sites, weights=None):
    """``pi`` (n, N, S + 1) -> (area (n, S + 1, G), bound (n, S + 1, G)): per region ``sum_i w_i pi_i`` in the device's order, and the
    bound of a second evaluation.  A region without a site: 0."""
    n, N, R = pi.shape
    w = np.ones(N) if weights is None else np.asarray(weights, dtype=np.float64)
    S = R - 1
    out, bound = np.zeros((n, R, len(sites))), np.zeros((n, R, len(sites)))
    for g, idx in enumerate(sites):
        if len(idx) == 0:
            continue
        terms = np.moveaxis(w[idx][None, :, None] * pi[:, idx, :], 1, -1)          # (n, R, N_g)
        runs = -(-len(idx) // 64)
        padded = np.full(terms.shape[:-1] + (runs * 64,), -0.0)
        padded[..., :len(idx)] = terms
        partial = wave_tree(padded.reshape(terms.shape[:-1] + (runs, 64)))          # (n, R, runs)
        total = partial[..., 0]
        for k in range(1, runs):
            total = total + partial[..., k]
        out[..., g] = total
        bound[..., g] = (8.0 * S + 2.0 * max(len(idx) - 1, 0)) * U * np.abs(terms).sum(axis=-1)
    return out, bound


def enumerate_pmf(psi32):
    """``psi32`` (S,) float32, S small -> the pmf by enumeration of all 2^S presence patterns in exact rational arithmetic, as floats'
    exact ``Fraction`` values (a list of S + 1 Fractions)."""
    from fractions import Fraction

    p = [Fraction(float(v)) for v in np.asarray(psi32, dtype=np.float32)]
    S = len(p)
    out = [Fraction(0)] * (S + 1)
    for pattern in range(1 << S):
        prob = Fraction(1)
        for s in range(S):
            prob *= p[s] if (pattern >> s) & 1 else 1 - p[s]
        out[bin(pattern).count("1")] += prob
    return out


def integer_quantiles(pmf_rows, probs):
    """The wrapper's rule, by the plainest loop: per q the smallest r with cumsum(pmf)[r] >= q, S where rounding leaves none."""
    pmf_rows = np.asarray(pmf_rows, dtype=np.float64)
    out = np.empty((len(probs),) + pmf_rows.shape[:-1], dtype=np.int64)
    for k, q in enumerate(probs):
        for idx in np.ndindex(*pmf_rows.shape[:-1]):
            cum, r = np.cumsum(pmf_rows[idx]), 0
            while r < len(cum) - 1 and not cum[r] >= q:
                r += 1
            out[(k,) + idx] = r
    return out


def check(got, psi32, regions_sites, weights, probs, label=""):
    """The wrapper's result against the definition on ``predict()``'s psi (n, N, S) float32.  Prints and returns the largest error as a
    fraction of its bound."""
    import totals_ref

    psi32 = np.asarray(psi32)
    n, N, S = psi32.shape
    assert got["n_species"] == S and got["n_draws"] == n and np.array_equal(got["probs"], np.asarray(probs, dtype=np.float64)), label
    worst = {}

    def within(name, value, want, bound):
        assert value.shape == want.shape and value.dtype == np.float64, (label, name, value.shape, want.shape)
        err = np.abs(value - want)
        ok = bound > 0
        worst[name] = float(np.max(err[ok] / bound[ok], initial=0.0))
        assert np.isfinite(value).all() and np.all(err <= bound), (label, name, float(err.max()), worst[name])

    pi, _ = pmf(psi32)
    assert_scaled(pi)
    if "site" in got:
        want_pmf, want_mean, want_sd = site_outputs(psi32)
        b_pmf, b_mean, b_sd = site_bounds(psi32, want_pmf, want_mean, want_sd)
        site = got["site"]
        within("pmf", site["pmf"], want_pmf, b_pmf)
        within("expected mean", site["expected"]["mean"], want_mean, b_mean)
        if n > 1:
            within("expected sd", site["expected"]["sd"], want_sd, b_sd)
        else:
            assert np.isnan(site["expected"]["sd"]).all(), label
        r = np.arange(S + 1, dtype=np.float64)
        assert np.array_equal(site["mean"], site["pmf"] @ r), label
        assert np.array_equal(site["quantiles"], integer_quantiles(site["pmf"], probs)) and site["quantiles"].dtype.kind == "i", label
        assert site["sd"].shape == (N,) and np.all(site["sd"] >= 0), label
    want_area, b_area = area(pi, regions_sites, weights)
    within("area", got["area"]["draws"], want_area, b_area)
    a = got["area"]["draws"]
    assert np.array_equal(got["at_least"]["draws"], np.cumsum(a[:, ::-1], axis=1)[:, ::-1]), label
    assert np.array_equal(got["richness"]["draws"], np.einsum("r,nrg->ng", np.arange(S + 1, dtype=np.float64), a)), label
    for name in ("area", "at_least", "richness"):
        totals_ref.check_summaries(got[name], probs, f"{label} {name}")
    top = max(worst.values())
    print(f"{label}: largest error as a fraction of its bound: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    return top
