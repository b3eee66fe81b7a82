"""The definition of ``regional_totals`` in NumPy, on ``predict()``'s arrays for the same seed: per draw and region, the float64 sum of
``w_i * (double) v_i`` over the region's sites -- ``np.sum(w[idx] * v[..., idx].astype(np.float64))`` --, and the bound within which
two float64 sums of the same terms agree.

The bound is derived, not measured.  Both sides add the same N_g float64 products, each in an order of its own (NumPy pairwise, the
device a tree per 64 sites and then the runs in order).  A sum of N_g terms in any order is off the exact sum by at most
(N_g - 1) u sum |term| to first order, u = 2^-53, so the two are at most ``2 (N_g - 1) 2^-53 sum_{i in g} |w_i v_i|`` apart.  With unit
weights the latent totals are sums of small integers, exact on both sides: equality."""
import numpy as np

U = 2.0 ** -53


def region_sites(regions, n_sites):
    """-> (labels, [the sites of every label in site order]); ``None``: one region ``"all"``; masked or NaN labels: in no region."""
    if regions is None:
        return np.array(["all"]), [np.arange(n_sites)]
    out = np.ma.getmaskarray(regions).reshape(-1).copy()
    lab = np.asarray(np.ma.getdata(regions)).reshape(-1)
    assert lab.size == n_sites
    if lab.dtype.kind == "f":
        out |= np.isnan(lab)
    labels = np.unique(lab[~out])
    return labels, [np.flatnonzero(~out & (lab == label)) for label in labels]


def totals(v, sites, weights=None):
    """``v`` (n, ..., N, S) -> (n, ..., G, S) float64: ``sum_{i in g} w_i (double) v_i`` per region, and the bound on a second sum of
    the same terms, same shape."""
    v = np.asarray(v)
    w = np.ones(v.shape[-2]) if weights is None else np.asarray(weights, dtype=np.float64)
    want, bound = [], []
    for idx in sites:
        terms = w[idx][:, None] * v[..., idx, :].astype(np.float64)
        want.append(np.sum(terms, axis=-2))
        bound.append(2.0 * max(len(idx) - 1, 0) * U * np.sum(np.abs(terms), axis=-2))
    return np.stack(want, axis=-2), np.stack(bound, axis=-2)


def brute_force(v, sites, weights=None):
    """The same by the plainest loop: one product and one addition at a time, in site order.  ``v`` (n, N)."""
    v = np.asarray(v)
    out = np.zeros((v.shape[0], len(sites)))
    for n in range(v.shape[0]):
        for g, idx in enumerate(sites):
            for i in idx:
                out[n, g] += (1.0 if weights is None else float(weights[i])) * float(v[n, i])
    return out


def check_summaries(entry, probs, label=""):
    """mean, sd (ddof 1, NaN for one draw) and quantiles (linear) are NumPy's on ``draws``."""
    d = entry["draws"]
    assert d.dtype == np.float64, label
    assert np.array_equal(entry["mean"], np.mean(d, axis=0)), label
    if d.shape[0] > 1:
        assert np.array_equal(entry["sd"], np.std(d, axis=0, ddof=1)), label
    else:
        assert entry["sd"].shape == d.shape[1:] and np.isnan(entry["sd"]).all(), label
    assert np.array_equal(entry["quantiles"], np.quantile(d, np.asarray(probs, dtype=np.float64), axis=0)), label
    assert entry["quantiles"].shape == (len(probs),) + d.shape[1:], label


def check(got, preds, first, second, regions, weights, probs, label="", latent=True):
    """The wrapper's result against the definition on ``predict()``'s arrays.  Returns the largest error as a fraction of its bound."""
    v = np.asarray(preds[first])                     # (n, T, N, S), constant over T
    n, T, N, S = v.shape
    labels, sites = region_sites(regions, N)
    G = len(sites)
    w = np.ones(N) if weights is None else np.asarray(weights, dtype=np.float64)
    assert np.array_equal(got["regions"], labels), label
    assert np.array_equal(got["n_sites"], [len(idx) for idx in sites]) and got["n_sites"].dtype.kind == "i", label
    for g, idx in enumerate(sites):   # (two float64 sums of the same weights: the bound above)
        assert abs(got["weight"][g] - w[idx].sum()) <= 2.0 * max(len(idx) - 1, 0) * U * np.abs(w[idx]).sum(), (label, g)
    assert got["n_draws"] == n and np.array_equal(got["probs"], np.asarray(probs, dtype=np.float64)), label
    assert set(got) == {"regions", "n_sites", "weight", "probs", "n_draws", first} | ({second} if latent else set()), label
    worst = 0.0
    pairs = [(first, v[:, 0], (n, G, S))] + ([(second, np.asarray(preds[second]), (n, T, G, S))] if latent else [])
    for name, values, shape in pairs:
        want, bound = totals(values, sites, weights)
        d = got[name]["draws"]
        assert d.shape == shape and d.dtype == np.float64, (label, name, d.shape)
        err = np.abs(d - want)
        assert np.isfinite(d).all() and np.all(err <= bound), (label, name, float(err.max()), float(bound.max()))
        if name == second and weights is None:
            assert np.array_equal(d, want), (label, name)   # integers below 2^53
        worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0)))
        check_summaries(got[name], probs, f"{label} {name}")
    return worst
