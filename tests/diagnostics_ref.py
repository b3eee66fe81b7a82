"""site_diagnostics' definition in NumPy on predict()'s arrays -- numpyro's effective sample size and split R-hat by direct lagged sums in
float64 -- and the bounds of the comparison; shared by tests/test_site_diagnostics_cpu.py and tests/test_gpu_site_diagnostics.py.

The definition, for a float32 array ``v32`` with the C n draws on axis 0, chain-major, ``x = v32.astype(float64).reshape(C, n, ...)``:
    m_c = mean_t x[c, t];   s2_c = sum_t (x[c, t] - m_c)^2 / (n - 1);   d = x - m_c
    W = mean_c s2_c;   plus = W (n - 1) / n;   C > 1: plus += var_c(m_c, ddof=1);   C == 1: W = plus
    gamma_k = mean_c (1 / n) sum_{t < n - k} d[c, t] d[c, t + k]
    rho_k = 1 - (W - gamma_k) / plus, rho_0 = 1;   P_p = rho_{2p} + rho_{2p+1}, p < n // 2
    tau = -1 + 2 (P_0 + sum_{p >= 1} cummin(max(P_p, 0)));   n_eff = C n / tau
    r_hat = sqrt(plus' / W') over the 2 C half chains x[:, :h], x[:, n - h:], h = n // 2
    mean = x.mean over all draws;   sd = x.std(ddof=1) over all draws                         (tests/summary_ref.py's)

Bounds (derived, not tuned).  The device states the same definition; it differs from this file in the order of its float64 sums and in
fusing a product into the addition that follows it.  With u = 2^-53 and, per cell, Q_c = sum_t d[c, t]^2, Wb = mean_c Q_c / n,
M = mean_c |m_c| sqrt(Q_c / n), B = var_c(m_c, ddof=1):
  - m_c is a sum of n values of one sign: |dm_c| <= n u |m_c| in any order.  A centred value inherits it: |dd| <= n u |m_c| + u |d|.
  - A lagged sum S = sum_t d_t d_{t+k} has sum |d_t d_{t+k}| <= Q_c (Cauchy-Schwarz): summing costs (n + 1) u Q_c, the perturbed factors
    2 |dm_c| sum |d| + 2 u Q_c with sum |d| <= sqrt(n Q_c).  Averaged over the chains, for every lag (lag 0, that is W, included):
        G = u ((n + C + 3) Wb + 2 n M)
  - B moves by dB = u (4 n max_c |m_c| sqrt(2 B) + (C + 3) B), and plus by G + dB.
  - rho_k = 1 - (W - gamma_k) / plus with |1 - rho_k| <= 4 (plus >= W (n - 1) / n, |gamma_k| <= W, n >= 2):
        R = (8 G + 4 dB) / plus + 15 u
  - A pair moves by E = 2 R + u max |P|.  Clipping at 0 and the running minimum are 1-Lipschitz, so EVERY term of tau moves by at most
    E -- also the terms behind the pair at which one side stops and the other, a rounding away, does not.  With the n // 2 terms summed:
        dtau = 2 (n // 2) E + 2 u (n // 2 + 2) (|P_0| + sum run)
  - n_eff = C n / tau:  |dn_eff| <= |n_eff| (r / (1 - r) + 4 u) with r = dtau / |tau|.  A cell with r >= 1 / 2 -- tau next to 0: always
    so for one chain of two draws, where P_0 = 1 / 2 and tau = 0 up to a rounding, n_eff +-inf or +-1e16 -- has no such bound and is
    compared through what is bounded there: |C n / got - C n / want| <= dtau + 4 u |tau|.
  - The first-order bound.  Where the stop is clear -- no pair up to and including the first one <= 0 lies within 2 E of 0 -- both sides
    clip the same pairs and stop at the same pair, and only the terms that enter tau move.  tau is the sum of -1, 2 P_0 and the 2 run_p,
    each a float64 sum of n terms in another order: |dn_eff| <= 8 n 2^-52 cond |n_eff| with the conditioning of that sum,
    cond = (1 + 2 (|P_0| + sum run_p)) / |tau|, and tests/summary_ref.py's margin of 8.  This is not a worst case (the cancellation in
    1 - (W - gamma_k) / plus and the chain means' |m| / sd do not enter it): it is the bound the estimator is expected to hold, and the
    one the cells with a clear stop are held to; the worst case above is kept for the others -- a pair next to 0, tau next to 0.
  - r_hat = sqrt(plus' / W'): relative error (G' / W' + (G' + dB') / plus') / 2 + 3 u, G' and dB' the above for the half chains.
  - Each side of a comparison carries that error: the bounds are twice the above.  No further margin: every step is a worst case.  They
    are of the order n^2 u, far looser than the first-order bound, and are what is left for the cells where that one has no answer
    (the pair at which the sequence stops lies next to 0); an indexing mistake (a lag short, a draw of the next chain) is of the
    order 1 / n.
  - Against values that are not the same bits (bench.py forms psi in float64 and rounds it; the device forms it in float32): with
    |dx| <= eps a centred value moves by 2 eps, a lagged sum over n by 4 eps mean_c sqrt(Q_c / n), B by 4 eps sqrt(2 B): G and dB grow
    by those terms and everything behind them follows (``reference(..., eps=)``).
  - mean rtol 1e-12 and sd |got - want| <= 1e-10 want + 1e-14 max(1, |mean|): tests/summary_ref.py's, for at most ~1100 draws.
NaN and infinity: where the definition gives NaN (0 / 0: a constant cell, a half of one draw) or an infinite r_hat (constant halves that
differ), the other side must give the same.  (An infinite n_eff is tau = 0 and goes through the reciprocal.)
"""
import warnings

import numpy as np

U = 2.0 ** -53
FIRST_ORDER_MARGIN = 8   # tests/summary_ref.py's margin over n 2^-5x for a float64 sum in another order
WORST = {"n_eff": 0.0, "r_hat": 0.0, "mean": 0.0, "sd": 0.0}   # the largest error seen, as a fraction of its bound (printed by every check)


def _chains(v32, n_chains):
    v32 = np.asarray(v32)
    assert v32.dtype == np.float32 and v32.shape[0] % n_chains == 0
    n = v32.shape[0] // n_chains
    return v32.astype(np.float64).reshape(n_chains, n, -1), v32.shape[1:]


def _within_plus(x):
    """x (C, n, m) -> W, plus, and what their bounds want: Wb, M, B, max |m_c|."""
    C, n, _ = x.shape
    m = x.sum(axis=1) / n
    d = x - m[:, None]
    Q = (d * d).sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        W = (Q / (n - 1)).sum(axis=0) / C
    plus = W * (n - 1) / n
    B = np.zeros_like(W)
    if C > 1:
        B = ((m - m.sum(axis=0) / C) ** 2).sum(axis=0) / (C - 1)
        plus = plus + B
    else:
        W = plus
    return d, W, plus, dict(Wb=(Q / n).sum(axis=0) / C, M=(np.abs(m) * np.sqrt(Q / n)).sum(axis=0) / C, B=B, mmax=np.abs(m).max(axis=0),
                            S=np.sqrt(Q / n).sum(axis=0) / C)


def _errors(n, C, c, eps=0.0):
    """G and dB of the module's docstring; ``eps``: the values themselves differ by up to that much between the two sides."""
    G = U * ((n + C + 3) * c["Wb"] + 2 * n * c["M"]) + 4 * eps * c["S"]
    dB = U * (4 * n * c["mmax"] * np.sqrt(2 * c["B"]) + (C + 3) * c["B"]) + 4 * eps * np.sqrt(2 * c["B"]) if C > 1 else np.zeros_like(G)
    return G, dB


def reference(v32, n_chains, eps=0.0):
    """n_eff, r_hat, mean, sd of the definition; and the bounds of n_eff, r_hat and C n / n_eff (``tau``) -- absolute, both sides' errors
    -- with ``live``, the pairs of the cell that enter tau with more than zero (P_0 among them).  ``v32`` (C n, ...) float32, chain-major.
    Direct lagged sums: O(n^2) per cell.  ``eps``: the other side's values differ from ``v32`` by up to that much (the docstring's last
    bound)."""
    x, tail = _chains(v32, n_chains)
    C, n, m = x.shape
    assert n >= 2
    with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"):
        warnings.simplefilter("ignore")
        d, W, plus, c = _within_plus(x)
        K = 2 * (n // 2)
        rho = np.empty((K, m))
        rho[0] = 1.0
        for k in range(1, K):
            gamma = (d[:, :n - k] * d[:, k:]).sum(axis=1).sum(axis=0) / C / n
            rho[k] = 1.0 - (W - gamma) / plus
        P = rho[0::2] + rho[1::2]
        run = np.minimum.accumulate(np.where(np.isnan(P[1:]), np.nan, np.maximum(P[1:], 0.0)), axis=0)
        total = P[0] + run.sum(axis=0)
        tau = -1.0 + 2.0 * total
        n_eff = C * n / tau
        G, dB = _errors(n, C, c, eps)
        R = (8 * G + 4 * dB) / plus + 15 * U
        E = 2 * R + U * np.abs(P).max(axis=0)
        dtau = 2 * (n // 2) * E + 2 * U * (n // 2 + 2) * (np.abs(P[0]) + run.sum(axis=0))
        r = dtau / np.abs(tau)
        b_n_eff = 2 * np.abs(n_eff) * np.where(r < 0.5, r / (1 - r) + 4 * U, np.inf)
        b_tau = 2 * (dtau + 4 * U * np.abs(tau))   # of C n / n_eff, where n_eff has no bound
        # the first-order bound, where the stop is clear: no pair up to and including the first one <= 0 lies within both sides' error
        # of 0, so both sides clip and stop at the same pairs and only the terms that enter tau move
        before = np.logical_and.accumulate(P[1:] > 0, axis=0)
        upto = np.concatenate([np.ones((1, m), dtype=bool), before[:-1]], axis=0) if n // 2 > 1 else before
        clear = ~((np.abs(P[1:]) <= 2 * E) & upto).any(axis=0) & (r < 0.5)
        cond = (1.0 + 2.0 * (np.abs(P[0]) + run.sum(axis=0))) / np.abs(tau)
        b_first = FIRST_ORDER_MARGIN * n * 2.0 ** -52 * cond * np.abs(n_eff)
        if eps == 0.0:
            b_n_eff = np.where(clear & (b_first < b_n_eff), b_first, b_n_eff)

        h = n // 2
        halves = np.concatenate([x[:, :h], x[:, n - h:]], axis=0)
        _, Wh, plus_h, ch = _within_plus(halves)
        r_hat = np.sqrt(plus_h / Wh)
        Gh, dBh = _errors(h, 2 * C, ch, eps)
        b_r_hat = 2 * np.abs(r_hat) * ((Gh / Wh + (Gh + dBh) / plus_h) / 2 + 3 * U)

        flat = x.reshape(C * n, m)
        mean, sd = flat.mean(axis=0), flat.std(axis=0, ddof=1)
    shape = lambda a: a.reshape(tail)
    return dict(n_eff=shape(n_eff), r_hat=shape(r_hat), mean=shape(mean), sd=shape(sd)), dict(n_eff=shape(b_n_eff), r_hat=shape(b_r_hat), tau=shape(b_tau), first_order=shape(clear & (eps == 0.0)), live=shape(1 + (run > 0).sum(axis=0)))


def _fraction(got, want, bound, label, key):
    """max |got - want| / bound over the cells where the definition is finite; NaN and infinity must agree."""
    got, want = np.broadcast_arrays(np.asarray(got), want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{key} {label}: NaN where the definition has none, or none where it has"
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), f"{key} {label}: infinite cells"
    fin = np.isfinite(want)
    assert np.all(np.isfinite(bound[fin])), f"{key} {label}: a cell without a bound"
    err = np.abs(got[fin] - want[fin])
    return float(np.max(err / np.where(bound[fin] > 0, bound[fin], 1.0), initial=0.0)), bool(np.all(err <= bound[fin]))


def _fraction_n_eff(got, want, bound, bound_tau, total, label):
    """The same for n_eff; the cells without a bound of their own (tau next to 0) through total / n_eff."""
    got, want = np.broadcast_arrays(np.asarray(got), want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"n_eff {label}: NaN where the definition has none, or none where it has"
    well = np.isfinite(bound)
    ill = ~well & ~np.isnan(want)
    with np.errstate(divide="ignore"):
        err = np.concatenate([np.abs(got[well] - want[well]), np.abs(total / got[ill] - total / want[ill])])
    b = np.concatenate([bound[well], bound_tau[ill]])
    assert np.all(np.isfinite(b)) and np.all(np.isfinite(err)), f"n_eff {label}: a cell without a bound"
    return float(np.max(err / np.where(b > 0, b, 1.0), initial=0.0)), bool(np.all(err <= b))


def check(got, v32, n_chains, label=""):
    """One site's ``{"n_eff", "r_hat", "mean", "sd", "mcse_mean"}`` (any shape that broadcasts from the definition's) against the
    definition at the bounds of the module's docstring; prints the largest errors as fractions of their bounds."""
    want, bound = reference(v32, n_chains)
    for k in ("n_eff", "r_hat", "mean", "sd", "mcse_mean"):
        assert got[k].dtype == np.float64 and got[k].shape == want["mean"].shape, (label, k, got[k].shape, want["mean"].shape)
    bound["mean"] = 1e-12 * np.abs(want["mean"])
    bound["sd"] = 1e-10 * want["sd"] + 1e-14 * np.maximum(1.0, np.abs(want["mean"]))
    frac, ok = {}, {}
    C, n = n_chains, np.asarray(v32).shape[0] // n_chains
    for k in WORST:
        frac[k], ok[k] = _fraction_n_eff(got[k], want[k], bound[k], bound["tau"], C * n, label) if k == "n_eff" else _fraction(got[k], want[k], bound[k], label, k)
        WORST[k] = max(WORST[k], frac[k])
    print(f"{label:44s} {C} x {n:4d} cells {want['mean'].size:7d} ({int(bound['first_order'].sum())} at the first-order bound)  of its bound: " + "  ".join(f"{k} {frac[k]:.2e}" for k in WORST)
          + "   (worst so far " + " ".join(f"{WORST[k]:.2e}" for k in WORST) + ")")
    for k in WORST:
        assert ok[k], f"{k} {label}"
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(got["mcse_mean"], got["sd"] / np.sqrt(got["n_eff"]), equal_nan=True), f"mcse_mean {label}"
    return want
