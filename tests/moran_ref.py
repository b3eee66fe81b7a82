"""The definition of ``residual_moran`` in NumPy float64 (TEST INFRASTRUCTURE), on ``predict()``'s and ``conditional_occupancy()``'s
arrays, with the masks recomputed from the data, and the bounds within which a second float64 evaluation agrees.  The bounds are
derived, not measured; ``u = 2^-53``.

Per one species, posterior draw ``n``, period ``t``, site ``i`` (include/biolith_hip.h: bl_residual_moran):

* ``psi`` (n, T, N) and ``p`` (n, J, T, N) are ``predict()``'s float32 ``psi`` and ``prob_detection``; ``z`` is
  ``conditional_occupancy()``'s for the seed; ``z'`` and ``y'`` are ``predict()``'s ``z`` and ``y`` for the replicate's seed;
* a visit is *seen* where the observation, the visit's covariates and the site's covariates are all present; ``s`` counts them;
* occupancy: ``o = z - psi``, replicate ``o' = z' - psi``, every site in the field;
* detection: ``d = (sum_{j seen} (y_j - p_j)) / s`` in visit order, in the field where ``z = 1 and s > 0``; the replicate with ``y'``
  and ``z'`` over the same seen visits;
* Moran's I of a masked field (v, m) over the CSR graph: ``M = sum m``, ``mu = sum m v / M``, ``c = v - mu``,
  ``num = sum_i m_i c_i s_i`` with ``s_i = sum_{e in row i} w_e m_j c_j`` in CSR order, ``den = sum_i m_i c_i^2``,
  ``W = sum_i m_i sum_e w_e m_j``, ``I = (M / W) num / den`` left to right; NaN where ``M < 2``, ``W == 0`` or ``max == min``.

The sums over sites are in the device's order all the same -- runs of 64 sites, the tree over lanes 32, 16, .. 1 apart with -0.0 where a
site is outside the field or past the last one, the runs in order --, so the two evaluations usually agree to the bit; the bounds below
do not rely on it.

Bounds (two evaluations that may order every sum otherwise; first order, times ``SAFETY`` for the second).  A sum of K terms is within
``(K - 1) u sum |terms|`` of exact, two of them within twice that.

* ``mu``:   ``e_mu = (2 (M - 1) + 2) u sum_i m_i |v_i| / M``                          (the sum, the division)
* ``c_i``:  ``e_c(i) = e_mu + 2 u |c_i|``
* ``s_i``:  ``e_s(i) = sum_e |w_e| m_j e_c(j) + 2 (deg_i + 1) u sum_e |w_e c_j| m_j``  (the products, the row's sum)
* ``num``:  ``e_num = sum_i m_i (e_c(i) |s_i| + |c_i| e_s(i) + 2 u |c_i s_i|) + 2 (M - 1) u sum_i m_i |c_i s_i|``
* ``den``:  ``e_den = sum_i m_i (2 |c_i| e_c(i) + 2 u c_i^2) + 2 (M - 1) u den``
* ``W``:    ``e_W = 2 u sum_i m_i deg_i sum_e |w_e| m_j + 2 (M - 1) u sum_i m_i |W_i|``
* ``I``:    ``|I| (e_W / |W| + e_den / den + 6 u) + (M / |W|) e_num / den``

``I`` is O(1), so a compared case must give a bound below ``BOUND_CAP = 1e-9``: ``check`` asserts it -- a case with a larger bound
(a field all but constant, weights that all but cancel) is a badly chosen input and is replaced, not skipped.

Site means.  ``occ_mean`` is the sum of n terms in draw order over n: ``(2 (n - 1) + 2) u sum_n |o| / n``; ``det_mean`` the same over
the draws that have the site in the field, each ``d`` itself within ``2 (s + 1) u sum_j |y_j - p_j| / s`` (J exact differences,
their sum, the division); ``n_occupied`` and the fields' sizes are integers: equality.
"""
import numpy as np

import pred_rng_ref

U = 2.0 ** -53
SAFETY = 1.01
BOUND_CAP = 1e-9
FIELDS = ("occupancy", "occupancy_rep", "detection", "detection_rep")


# ------------------------------------------------------------------------------------------ the fields ----
def seen_visits(obs, obs_covs, site_covs):
    """(N, T, J) bool: the visits that enter the likelihood (``_conditional._unmasked``'s rule), one species' ``obs`` (N, T, J)."""
    site_nan = np.isnan(np.asarray(site_covs, dtype=np.float64)).any(-1)
    return ~(np.isnan(obs) | np.isnan(np.asarray(obs_covs, dtype=np.float64)).any(-1) | site_nan[:, None, None])


def fields(psi, p, z, z_rep, y_rep, obs, seen):
    """The four fields (4, n, T, N) float64, NaN outside a field's mask, and the bound of each detection value.  ``psi`` (n, T, N) and
    ``p`` (n, J, T, N) float32; ``z``, ``z_rep`` (n, T, N); ``y_rep`` (n, J, T, N); ``obs`` (N, T, J) with NaN; ``seen`` (N, T, J)."""
    assert np.asarray(psi).dtype == np.float32 and np.asarray(p).dtype == np.float32
    psi, p = np.asarray(psi, dtype=np.float64), np.asarray(p, dtype=np.float64)
    z, z_rep, y_rep = (np.asarray(a, dtype=np.float64) for a in (z, z_rep, y_rep))
    n, J = p.shape[0], p.shape[1]
    ok = np.asarray(seen).transpose(2, 1, 0)                                 # (J, T, N)
    y = np.nan_to_num(np.asarray(obs, dtype=np.float64)).transpose(2, 1, 0)  # (J, T, N)
    s = ok.sum(0)                                                            # (T, N)
    so, sr, absum = np.zeros(psi.shape), np.zeros(psi.shape), np.zeros(psi.shape)
    for j in range(J):   # in visit order
        so = so + np.where(ok[j], y[j][None] - p[:, j], 0.0)
        sr = sr + np.where(ok[j], y_rep[:, j] - p[:, j], 0.0)
        absum = absum + np.where(ok[j], np.maximum(np.abs(y[j][None] - p[:, j]), np.abs(y_rep[:, j] - p[:, j])), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        d, dr = so / s[None], sr / s[None]
        e_d = 2.0 * (s[None] + 1) * U * absum / s[None]
    has = (s > 0)[None]
    v = np.stack([z - psi, z_rep - psi, np.where((z == 1) & has, d, np.nan), np.where((z_rep == 1) & has, dr, np.nan)])
    return v, np.where(np.isnan(e_d), 0.0, e_d)


# ------------------------------------------------------------------------------------------ Moran's I ----
def wave_sum(x):
    """``x`` (..., N) -> (...): runs of 64, the last filled with -0.0, the tree over lanes 32, 16, .. 1 apart, the runs in order."""
    N = x.shape[-1]
    runs = -(-N // 64)
    padded = np.full(x.shape[:-1] + (runs * 64,), -0.0)
    padded[..., :N] = x
    t = padded.reshape(x.shape[:-1] + (runs, 64))
    o = 32
    while o:
        t = t[..., :o] + t[..., o:2 * o]
        o //= 2
    t = t[..., 0]
    total = t[..., 0]
    for k in range(1, runs):
        total = total + t[..., k]
    return total


def _rows(graph, N):
    indptr, indices, data = graph
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    data = np.ones(indices.size) if data is None else np.asarray(data, dtype=np.float64)
    assert indptr.size == N + 1
    return indptr, indices, data, np.diff(indptr)


def moran(v, graph):
    """Moran's I of the masked field ``v`` (..., N), NaN = outside -> (I (...), M (...) int, bound (...))."""
    v = np.asarray(v, dtype=np.float64)
    N = v.shape[-1]
    indptr, indices, data, deg = _rows(graph, N)
    m = ~np.isnan(v)
    neg0 = lambda x: np.where(m, x, -0.0)
    M = m.sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = wave_sum(neg0(v)) / M
        c = np.where(m, v - mu[..., None], 0.0)            # (0 outside the field: its terms below are +0, the sum's identity from +0)
        e_mu = (2.0 * (M - 1) + 2.0) * U * np.where(m, np.abs(v), 0.0).sum(-1) / M
    e_c = np.where(m, e_mu[..., None] + 2.0 * U * np.abs(c), 0.0)
    s, Wi = np.zeros(v.shape), np.zeros(v.shape)
    sa, e_in, wabs = np.zeros(v.shape), np.zeros(v.shape), np.zeros(v.shape)
    for r in range(int(deg.max(initial=0))):   # the r-th entry of every row that has one: CSR order
        rows = np.flatnonzero(deg > r)
        e = indptr[rows] + r
        j, w = indices[e], data[e]
        mj = m[..., j]
        term = np.where(mj, w * c[..., j], 0.0)
        s[..., rows] = s[..., rows] + term
        Wi[..., rows] = Wi[..., rows] + np.where(mj, w, 0.0)
        sa[..., rows] += np.abs(term)
        e_in[..., rows] += np.abs(w) * e_c[..., j]
        wabs[..., rows] += np.where(mj, np.abs(w), 0.0)
    cs = c * s
    num, den, W = wave_sum(neg0(cs)), wave_sum(neg0(c * c)), wave_sum(neg0(Wi))
    e_s = e_in + 2.0 * (deg + 1) * U * sa
    Mm1 = np.maximum(M - 1, 0)
    e_num = (m * (e_c * np.abs(s) + np.abs(c) * e_s + 2.0 * U * np.abs(cs))).sum(-1) + 2.0 * Mm1 * U * (m * np.abs(cs)).sum(-1)
    e_den = (m * (2.0 * np.abs(c) * e_c + 2.0 * U * c * c)).sum(-1) + 2.0 * Mm1 * U * np.abs(den)
    e_W = 2.0 * U * (m * deg * wabs).sum(-1) + 2.0 * Mm1 * U * (m * np.abs(Wi)).sum(-1)
    big = np.where(m, v, -np.inf).max(-1, initial=-np.inf)
    small = np.where(m, v, np.inf).min(-1, initial=np.inf)
    undefined = (M < 2) | (W == 0.0) | (big == small)
    with np.errstate(invalid="ignore", divide="ignore"):
        I = (M / W) * num / den
        bound = SAFETY * (np.abs(I) * (e_W / np.abs(W) + e_den / den + 6.0 * U) + (M / np.abs(W)) * e_num / den)
    return np.where(undefined, np.nan, I), M.astype(np.int64), np.where(undefined, 0.0, bound)


def site_means(v, e_d):
    """The site outputs of the fields (4, n, T, N): (occ_mean, det_mean, n_occupied) and the bounds of the two means, one accumulator
    per cell in ascending draw order."""
    n = v.shape[1]
    o, d = v[0], v[2]
    inside = ~np.isnan(d)
    osum, dsum = np.zeros(o.shape[1:]), np.zeros(o.shape[1:])
    for k in range(n):
        osum = osum + o[k]
        dsum = dsum + np.where(inside[k], d[k], 0.0)
    cnt = inside.sum(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        det_mean = np.where(cnt > 0, dsum / cnt, np.nan)
        b_det = ((2.0 * np.maximum(cnt - 1, 0) + 2.0) * U * np.where(inside, np.abs(d), 0.0).sum(0) + np.where(inside, e_d, 0.0).sum(0)) / cnt
    b_occ = (2.0 * (n - 1) + 2.0) * U * np.abs(o).sum(0) / n
    return osum / n, det_mean, cnt.astype(np.int64), b_occ, np.where(cnt > 0, b_det, 0.0)


def p_value(obs, rep):
    """The share of the draws (axis 0) with both I finite in which I_rep >= I_obs; NaN if none."""
    ok = np.isfinite(obs) & np.isfinite(rep)
    k = ok.sum(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (ok & (rep >= obs)).sum(0) / np.where(k > 0, k, np.nan), k


# ------------------------------------------------------------------------------------------ the comparison ----
def _within(name, got, want, bound, label):
    """NaN positions agree exactly; elsewhere |got - want| <= bound.  Returns the largest error as a fraction of its bound."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (label, name, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (label, name, "NaN positions differ")
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    b = np.broadcast_to(bound, want.shape)[ok]
    assert np.all(err <= b), (label, name, float(err.max(initial=0.0)), float(b[err > b].min(initial=np.inf)))
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = np.where(err == 0.0, 0.0, err / b)
    return float(frac.max(initial=0.0))


def check_species(got, psi, p, z, z_rep, y_rep, obs, obs_covs, site_covs, graph, label="", block=64):
    """One species' outputs ``got`` = (moran_occ (n, T, 2), moran_det (n, T, 2), det_sites (n, T, 2), occ_mean (T, N), det_mean (T, N),
    n_occupied (T, N)), ``None`` = not compared, against the definition.  Prints and returns the largest error as a fraction of its
    bound."""
    v, e_d = fields(psi, p, z, z_rep, y_rep, obs, seen_visits(obs, obs_covs, site_covs))
    worst = 0.0
    m_occ, m_det, sites, o_mean, d_mean, n_occ = got
    if m_occ is not None or m_det is not None or sites is not None:
        for f, name in enumerate(FIELDS):
            parts = [moran(v[f, a:a + block], graph) for a in range(0, v.shape[1], block)]   # (blocks of draws: the temporaries stay small)
            I, M, bound = (np.concatenate(x) for x in zip(*parts))
            assert np.all(bound < BOUND_CAP), (label, name, "a badly chosen case: the derived bound is", float(bound.max()))
            out = m_occ if f < 2 else m_det
            if out is not None:
                worst = max(worst, _within(name, out[..., f & 1], I, bound, label))
            if f >= 2 and sites is not None:
                assert np.array_equal(sites[..., f & 1], M), (label, name, "the field's sites")
    if o_mean is not None:
        want_o, want_d, cnt, b_occ, b_det = site_means(v, e_d)
        worst = max(worst, _within("occ_mean", o_mean, want_o, b_occ, label), _within("det_mean", d_mean, want_d, b_det, label))
        assert np.array_equal(n_occ, cnt), (label, "n_occupied")
    print(f"{label}: largest error {worst:.3g} of its bound")
    return worst


def check(got, preds, lat, data, graph, label=""):
    """The wrapper's result ``got`` against the definition on ``preds = predict(seed_rep)`` and ``lat = conditional_occupancy(seed)``,
    species by species (species ``sp``'s seeds are the wrappers' own rule); ``data`` holds ``site_covs``, ``obs_covs`` and ``obs``
    (S, N, T, J)."""
    S = np.asarray(preds["psi"]).shape[-1]
    obs = np.asarray(data["obs"], dtype=np.float32)
    obs = obs if obs.ndim == 4 else obs[None]
    worst = 0.0
    for sp in range(S):
        o, d = got["occupancy"], got["detection"]
        one = (np.stack([o["moran_obs"][..., sp], o["moran_rep"][..., sp]], -1), np.stack([d["moran_obs"][..., sp], d["moran_rep"][..., sp]], -1),
               np.stack([d["n_sites_obs"][..., sp], d["n_sites_rep"][..., sp]], -1), o["mean"][..., sp], d["mean"][..., sp],
               got["n_occupied"][..., sp])
        worst = max(worst, check_species(one, np.asarray(preds["psi"])[..., sp], np.asarray(preds["prob_detection"])[..., sp],
                                         np.asarray(lat["z"])[..., sp], np.asarray(preds["z"])[..., sp], np.asarray(preds["y"])[..., sp],
                                         obs[sp], data["obs_covs"], data["site_covs"], graph, f"{label} species {sp}"))
    for key in ("occupancy", "detection"):
        share, k = p_value(got[key]["moran_obs"], got[key]["moran_rep"])
        assert np.array_equal(got[key]["p_value"], share, equal_nan=True) and np.array_equal(got[key]["n_finite"], k), (label, key)
    return worst


# ------------------------------------------------------------------------------------------ a restatement without the device ----
def restate_plain(site_covs, obs_covs, obs, beta, alpha, seed, seed_rep):
    """Plain occu without the device, for choosing cases on the CPU: ``psi`` and ``p`` as float32 from float64 sigmoids, the
    conditional q in float64, and the three draws from the cells' generators (tests/pred_rng_ref.py) in the kernels' order -> (psi,
    p, z, z_rep, y_rep) shaped as ``fields`` takes them.  The device forms psi, p and q in float32, so a uniform that falls between
    the two roundings of a threshold gives another draw: this is the statistic's behaviour, not the device's bits."""
    X, Wc = np.nan_to_num(np.asarray(site_covs, dtype=np.float64)), np.nan_to_num(np.asarray(obs_covs, dtype=np.float64))
    beta, alpha = np.asarray(beta, dtype=np.float64), np.asarray(alpha, dtype=np.float64)
    n, (N, T, J) = beta.shape[0], Wc.shape[:3]
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    psi = np.broadcast_to(sig(beta[:, :1] + beta[:, 1:] @ X.T)[:, None, :], (n, T, N)).astype(np.float32)
    p = sig(alpha[:, 0][:, None, None, None] + np.einsum("itjk,nk->njti", Wc, alpha[:, 1:])).astype(np.float32)   # (n, J, T, N)
    ok = seen_visits(obs, obs_covs, site_covs).transpose(2, 1, 0)
    y = np.nan_to_num(np.asarray(obs, dtype=np.float64)).transpose(2, 1, 0)
    p64, psi64 = p.astype(np.float64), psi.astype(np.float64)
    like1 = np.where(ok[None], np.where(y[None] == 1, p64, 1.0 - p64), 1.0).prod(1)
    like0 = np.where(ok[None] & (y[None] == 1), 0.0, 1.0).prod(1)
    q = psi64 * like1 / (psi64 * like1 + (1.0 - psi64) * like0)
    z = (pred_rng_ref.cells(seed, np.arange(n), T, N).uniform() < q).astype(np.int64)
    rep = pred_rng_ref.cells(seed_rep, np.arange(n), T, N)
    z_rep = (rep.uniform() < psi64).astype(np.int64)
    y_rep = np.stack([(rep.uniform() < z_rep * p64[:, j]).astype(np.int64) for j in range(J)], axis=1)
    return psi, p, z, z_rep, y_rep


# ------------------------------------------------------------------------------------------ the two cases of the separation test ----
def separation_case(gradient, n=40):
    """A hand-made case on a 20 x 20 grid of sites, T = 1, J = 3, detection probability one half, and a posterior for the model
    WITHOUT any spatial term (an intercept and one noise covariate a side, coefficients near their data-generating values).  With
    ``gradient`` the data come from an occupancy probability that rises smoothly from west to east -- structure the model lacks --;
    without, from the constant the posterior states (data seeds chosen on the CPU, with ``restate_plain``, so that the occupancy
    field's p-value is 0 and 0.475: tests/test_residual_moran_cpu.py).  -> (data with ``obs`` (1, N, T, J), the sites dict of the posterior, coords)."""
    rng = np.random.default_rng(7 if gradient else 10)
    side = 20
    gx, gy = np.meshgrid(np.arange(side, dtype=np.float64), np.arange(side, dtype=np.float64), indexing="ij")
    coords = np.stack([gx.ravel(), gy.ravel()], axis=1)
    N, T, J = side * side, 1, 3
    psi_true = 1.0 / (1.0 + np.exp(-6.0 * (coords[:, 0] / (side - 1) - 0.5))) if gradient else np.full(N, 0.5)
    z_true = rng.random(N) < psi_true
    obs = ((rng.random((N, T, J)) < 0.5) & z_true[:, None, None]).astype(np.float32)
    data = dict(site_covs=rng.normal(size=(N, 1)).astype(np.float32), obs_covs=rng.normal(size=(N, T, J, 1)).astype(np.float32),
                obs=obs[None])
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    sites = dict(beta=f32(np.stack([rng.normal(0.0, 0.1, n), rng.normal(0.0, 0.05, n)], -1)[:, None, :]),
                 alpha=f32(np.stack([rng.normal(0.0, 0.1, n), rng.normal(0.0, 0.05, n)], -1)[:, None, :]))
    return data, sites, coords
