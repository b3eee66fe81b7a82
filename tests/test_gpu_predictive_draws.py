"""What the post-fit kernels SAMPLE, cell by cell, against tests/pred_rng_ref.py: the exact restatement of their generator
(csrc/pred_rng.hpp) and of their samplers, fed with hand-made draw matrices -- no fit is run.  A cell is one (draw, period, site).

Tier 1 (exact, no cell left out): where the kernel returns the float32 threshold it compares a uniform with, the draw must equal
``u < threshold`` in every cell: occu's z and y and occu_cs's z and f (``deterministic``), occu_comb's z and y_pc
(``deterministic_comb``), z of site_/score_/count_posterior (their ``z_prob``) and the last period of ``path_posterior`` (its
``z_prob``; T = 1: the whole path).  ``test_a_tie_is_not_a_success`` builds draws whose threshold EQUALS the cell's uniform: it is what
found bl_predict_kernel's psi one ulp off ``deterministic``'s in some cells (a float32 division the compiler lowered per call site).

Tier 2 (exact outside a band): where the threshold is composed inside the kernel the reference is run twice per cell, every
threshold moved down and then up by a derived bound of the float32 evaluation's error.  A cell is DECIDED when the two runs agree on
every output of the cell and on the number of uniforms it took; every decided cell must equal the device, and no case may leave more
than 1e-3 of its cells undecided (``test_undecided_share``: evaluated from the reference alone, it runs without a GPU).

The bands (u = 2^-24, float32's unit roundoff; the uniforms lie on the grid of u):
  linear predictor   s = b0 + sum_k x_k b_k (+ effects), k fused multiply-adds or adds, each rounding once relative to a partial sum
                     that is at most S = sum |terms|: |error| <= (k + 2) u S                                              (``lin_band``)
  __expf(x)          = v_exp_f32(x log2 e).  The guides give no accuracy for the transcendental instructions; the instruction set's
                     figure is 1 ulp = 2 u relative, the rounded product x log2(e) adds |x| u relative, and the bound is doubled:
                     relative error <= (|x| + 4) 2 u, plus the error dx of x itself                                        (``exp_rel``)
  sigmoid            1 / (1 + e): d sigmoid / dx <= 1/4 and d sigmoid / d log e <= 1/4, so (dx + (|x| + 4) 2 u) / 4, plus u for
                     1 + e and 2.5 ulp for the division (the build's -fno-hip-fp32-correctly-rounded-divide-sqrt): + 8 u (``sigmoid_band``)
  compositions       of k float32 operations on values in [0, 1] (z p; 1 - (1 - p)(1 - fc)(1 - fu), contracted or not): k u on top
                     of the operands' bands (their derivatives are at most 1)
  __powf(q, N)       = exp2(N log2 q): 1 ulp each for log2 and exp2 and u for the product move q^N by at most
                     q^N |ln q^N| 4 u + q^N (2 N u + 4 u) <= (4 / e + 4) u + q^N 2 N u, and q's own band enters with N q^(N-1)
  Poisson rate       dur (exp(nu) + f): relative, the larger of exp_rel(nu) and exp_rel(phi), + 2 u (the rate is formed in float64)
  truncated Poisson  float64 inversion of a float32 eta: the reference runs at eta -/+ its lin_band
  conditionals       abundance_posterior's cdf, score_posterior's r_j, count_posterior's rho_j, path_posterior's backward kernels: the
                     allowances the existing parity tests hold these kernels to (tests/*_ref.py: bounds, at the families' committed
                     rtol), a quarter of the log-odds' allowance plus one ulp of 1
Samplers that take a data-dependent number of uniforms (the Poisson sampler; the binomial given a drawn N) make the rest of their
cell undecided once a visit is: the two runs have left the common stream.  A band of ~1e-6 leaves ~1e-5 of the cells undecided.

Scores (predictive_scores, predictive_comb) are floats: on decided cells they are compared with the float64 Box-Muller value.
Measured on an MI355X: max |s - s_ref| / sigma = 1.9e-6 (occu_cs 1.5e-6, occu_comb 1.9e-6; every case prints its own); the tolerance is
four times that, 7.6e-6, and by rule never above 1e-4 -- a misplaced uniform moves a score by order 1.
"""
import functools
import itertools
import math

import numpy as np
import pytest

import abundance_ref as A
import counts_ref as CR
import dyn_path_ref as DP
import latent_ref as L
import pred_rng_ref as R
import scores_ref as SR

U = 2.0 ** -24
CAP = 1e-3
MEASURED_SCORE_ERROR = 1.9e-6          # the largest over this module's six score cases on an MI355X (occu_comb, 2 / 3 / 1 visits)
SCORE_TOL = min(4 * MEASURED_SCORE_ERROR, 1e-4)
RTOL_CONDITIONAL = 2e-6                # tests/test_gpu_abundance.py, test_gpu_scores.py, test_gpu_counts.py: the families' bound

gpu = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------- the bands ----
def lin_band(S, k):
    return (k + 2) * U * S


def exp_rel(x, dx):
    return dx + (np.abs(x) + 4.0) * 2 * U


def sigmoid_band(x, dx):
    return 0.25 * (dx + (np.abs(x) + 4.0) * 2 * U) + 8 * U


def _sig(x):
    return np.exp(-np.logaddexp(0.0, -np.asarray(x, dtype=np.float64)))


def _f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------- data and predictors ----
def _covs(rng, N, T, J, Ks, Ko):
    return rng.normal(size=(N, Ks)).astype(np.float32), rng.normal(size=(N, T, J, Ko)).astype(np.float32)


def _theta(rng, n, D, Ks, Ko):
    """Intercepts in (-1, 1), slopes in (-0.7, 0.7), everything behind the coefficients (rates, log sds, effects) in (-0.6, 0.6)."""
    th = rng.uniform(-0.6, 0.6, size=(n, D))
    th[:, :Ks + Ko + 2] = rng.uniform(-0.7, 0.7, size=(n, Ks + Ko + 2))
    th[:, 0], th[:, Ks + 1] = rng.uniform(-1, 1, size=n), rng.uniform(-1, 1, size=n)
    return th.astype(np.float32)


def _predictors(X, W, th, lay, al0=None):
    """float64 eta (n, N), nu (n, J, T, N) of draws th (n, D) with the sums of the absolute values of their terms; ``lay``: the
    offsets of the effects (latent_ref.occu_theta_layout); visit v = t J + j of site i has its effect at o_e + i T J + v."""
    X, W, th = _f64(X), _f64(W), _f64(th)
    N, T, J, ko = W.shape
    Ks = X.shape[1]
    al0 = Ks + 1 if al0 is None else al0
    beta, alpha = th[:, :Ks + 1], th[:, al0:al0 + ko + 1]
    eta = beta[:, :1] + beta[:, 1:] @ X.T
    S_eta = np.abs(beta[:, :1]) + np.abs(beta[:, 1:]) @ np.abs(X).T
    nu = alpha[:, 0][:, None, None, None] + np.einsum("itjk,nk->njti", W, alpha[:, 1:])
    S_nu = np.abs(alpha[:, 0])[:, None, None, None] + np.einsum("itjk,nk->njti", np.abs(W), np.abs(alpha[:, 1:]))
    if lay is not None and lay["u"] >= 0:
        u, v = th[:, lay["u"]:lay["u"] + N], th[:, lay["v"]:lay["v"] + N]
        eta, S_eta = eta + u, S_eta + np.abs(u)
        nu, S_nu = nu + v[:, None, None, :], S_nu + np.abs(v)[:, None, None, :]
    if lay is not None and lay["e"] >= 0:
        e = th[:, lay["e"]:lay["e"] + N * T * J].reshape(-1, N, T, J).transpose(0, 3, 2, 1)
        nu, S_nu = nu + e, S_nu + np.abs(e)
    return eta, S_eta, nu, S_nu


class Case:
    """One handle, one draw matrix, one seed: what the reference and the device are both given."""

    def __init__(self, name, family, N, T, J, Ks, Ko, n, seed, **opt):
        self.name, self.family, self.seed, self.opt = name, family, seed, opt
        self.N, self.T, self.J, self.Ks, self.Ko, self.n = N, T, J, Ks, Ko, n

    def __repr__(self):
        return self.name


def _latent_threshold(eta3, d_eta3, rng, sign, K=0, abundance=False):
    if abundance:
        return R.truncated_poisson(rng, eta3 + sign * d_eta3, K)
    return (rng.uniform() < _sig(eta3) + sign * sigmoid_band(eta3, d_eta3)).astype(np.int64)


# --------------------------------------------------------------------------------- bl_predict (occu, occu_fp, occu_re, occu_rn) ----
def _setup_plain(c):
    o = c.opt
    rng = np.random.default_rng(1000 + c.N * 7 + c.T * 3 + c.J + c.Ks * 11 + c.Ko * 13)
    X, W = _covs(rng, c.N, c.T, c.J, c.Ks, c.Ko)
    fp = o.get("fp_mode") is not None
    lay = L.occu_theta_layout(c.N, c.T, c.J, c.Ks, c.Ko, fp, o.get("site_re", False), o.get("obs_re", False))
    th = _theta(rng, c.n, lay["D"], c.Ks, c.Ko)
    return rng, X, W, lay, th


def _make_predict(c):
    rng, X, W, lay, th = _setup_plain(c)
    o = c.opt
    if o.get("K") and c.n >= 2:          # one draw whose exp(eta) is above 745: exp(-lambda) = 0, the draw must be K
        th[1, :c.Ks + 1] = 0.0
        th[1, 0] = 8.0
    if o.get("model") in ("occu_rn", "nmixture"):
        th[:, 0] += 0.5
    return dict(X=X, W=W, lay=lay, th=th)


def _ref_predict(c, d, sign):
    o = c.opt
    eta, S_eta, nu, S_nu = _predictors(d["X"], d["W"], d["th"], d["lay"])
    th = _f64(d["th"])
    shape = (c.n, c.T, c.N)
    eta3, d_eta3 = np.broadcast_to(eta[:, None, :], shape), np.broadcast_to(lin_band(S_eta, c.Ks + 1)[:, None, :], shape)
    rng = R.cells(c.seed, np.arange(c.n), c.T, c.N)
    rn = o.get("model") == "occu_rn"
    lat = _latent_threshold(eta3, d_eta3, rng, sign, o.get("K", 0), abundance=rn)
    fpm = o.get("fp_mode")
    f, bf = 0.0, 0.0
    if fpm is not None:
        phi = th[:, d["lay"]["fp"]][:, None, None]
        f, bf = _sig(phi), sigmoid_band(phi, 0.0)
    y = np.empty((c.n, c.J, c.T, c.N), dtype=np.int64)
    for j in range(c.J):
        x, dx = nu[:, j], lin_band(S_nu[:, j], c.Ko + 2)
        r, br = _sig(x), sigmoid_band(x, dx)
        if rn:
            q = 1.0 - r
            pw = np.where(lat > 0, q ** lat, 1.0)
            b = np.where(lat > 0, lat * q ** np.maximum(lat - 1, 0) * (br + U) + (4 / math.e + 4) * U + pw * lat * 2 * U + U, 0.0)
            pd = 1.0 - pw
            if fpm is not None:
                pd, b = 1.0 - (1.0 - pd) * (1.0 - f), b + bf + 3 * U
        elif fpm is not None:
            fc, fu = (f, 0.0) if fpm == "constant" else (0.0, f)
            pd = 1.0 - (1.0 - lat * r) * (1.0 - fc) * (1.0 - np.where(lat > 0, 0.0, fu))
            b = lat * br + bf + 6 * U
        else:
            pd, b = lat * r, lat * br
        y[:, j] = rng.uniform() < pd + sign * b
    checks = [("exp(eta) > 745: the draw is K", bool((lat[1] == o["K"]).all()))] if rn and c.n >= 2 else []
    return dict(latent=lat, y=y), rng.taken, dict(checks=checks)


def _handle_predict(c, d):
    """The case's handle: its observations where it has some (the conditional posteriors), else all withheld."""
    from biolith_amd.engine import OccuDataset

    o = c.opt
    obs = d["Y"][None] if "Y" in d else np.full((1, c.N, c.T, c.J), np.nan, dtype=np.float32)
    model = o.get("model", "occu")
    effects = dict(site_random_effects=o.get("site_re", False), obs_random_effects=o.get("obs_re", False))
    kw = dict(model=model)
    if model == "occu_fp":
        kw.update(fp_mode=o["fp_mode"])
    elif model == "occu_re":
        kw.update(re_fp_mode=o.get("fp_mode"), **effects)
    elif model in ("occu_rn", "nmixture"):
        kw.update(max_abundance=o["K"], **effects)
        if o.get("fp_mode") is not None:
            kw["re_fp_mode"] = o["fp_mode"]
    elif model == "occu_cop":
        kw.update(fp_mode=o.get("fp_mode"), session_duration=d["dur"], **effects)
    ds = OccuDataset(d["X"], d["W"], obs, **kw)
    assert ds.D == d["th"].shape[1], (ds.D, d["th"].shape)
    return ds


def _device_predict(c, d):
    ds = _handle_predict(c, d)
    lat, y = ds.predictive(d["th"], seed=c.seed)
    # every subset of the wanted outputs gives the bytes of the full call
    assert np.array_equal(ds.predictive(d["th"], seed=c.seed, latent=False)[1], y)
    assert np.array_equal(ds.predictive(d["th"], seed=c.seed, y=False)[0], lat)
    ds.close()
    return dict(latent=lat, y=y)


# -------------------------------------------------------------------------------------- bl_predict_counts (nmixture, occu_cop) ----
def _make_counts(c):
    rng, X, W, lay, th = _setup_plain(c)
    o = c.opt
    d = dict(X=X, W=W, lay=lay, th=th)
    if o["model"] == "nmixture":
        th[:, 0] += 0.5
        if c.n >= 2:
            th[1, :c.Ks + 1] = 0.0
            th[1, 0] = 8.0
    else:
        # visit rates on both sides of 10 within the case: exp(nu) in about (2, 25), sessions of 0.5 .. 3
        th[:, c.Ks + 1] = rng.uniform(1.0, 3.0, size=c.n).astype(np.float32)
        th[:, c.Ks + 2:c.Ks + c.Ko + 2] *= 0.3
        d["dur"] = rng.uniform(0.5, 3.0, size=(c.N, c.T, c.J)).astype(np.float32)
        if o.get("fp_mode") is None and c.n >= 2:   # one draw with every rate 0: z = 0 everywhere, no false-positive rate
            th[1, :c.Ks + 1] = 0.0
            th[1, 0] = -60.0
    return d


def _ref_counts(c, d, sign):
    o = c.opt
    eta, S_eta, nu, S_nu = _predictors(d["X"], d["W"], d["th"], d["lay"])
    th = _f64(d["th"])
    shape = (c.n, c.T, c.N)
    eta3, d_eta3 = np.broadcast_to(eta[:, None, :], shape), np.broadcast_to(lin_band(S_eta, c.Ks + 1)[:, None, :], shape)
    rng = R.cells(c.seed, np.arange(c.n), c.T, c.N)
    nmix = o["model"] == "nmixture"
    lat = _latent_threshold(eta3, d_eta3, rng, sign, o.get("K", 0), abundance=nmix)
    fpm = o.get("fp_mode")
    f, rel_f = 0.0, 0.0
    if not nmix and fpm is not None:
        phi = th[:, d["lay"]["fp"]][:, None, None]
        f, rel_f = np.exp(phi), exp_rel(phi, 0.0)
    y = np.empty((c.n, c.J, c.T, c.N), dtype=np.int64)
    rates = []
    for j in range(c.J):
        x, dx = nu[:, j], lin_band(S_nu[:, j], c.Ko + 2)
        if nmix:
            y[:, j] = R.binomial(rng, lat, _sig(x) + sign * sigmoid_band(x, dx))
            continue
        dur = _f64(d["dur"])[:, :, j].T[None]                                       # (1, T, N)
        f_c, f_u = (f, 0.0) if fpm == "constant" else (0.0, f)
        rate = dur * (np.where(lat > 0, np.exp(x), f_u) + f_c)
        rel = np.maximum(np.where(lat > 0, exp_rel(x, dx), 0.0), rel_f) + 2 * U
        y[:, j] = R.poisson(rng, rate * (1.0 + sign * rel))[0]
        rates.append(rate)
    if nmix:
        checks = [("exp(eta) > 745: the draw is K", bool((lat[1] == o["K"]).all()))] if c.n >= 2 else []
    else:
        rates = np.stack(rates, axis=1)
        live = rates[rates > 0]
        checks = [("visit rates on both sides of 10", bool((live < 10).mean() > 0.1 and (live >= 10).mean() > 0.1))]
        if fpm is None and c.n >= 2:
            checks.append(("one draw with every rate 0", bool((rates[1] == 0).all() and (y[1] == 0).all())))
    return dict(latent=lat, y=y), rng.taken, dict(checks=checks)


# -------------------------------------------------------------------------------------------- bl_predict_scores (occu_cs) ----
def _make_scores(c):
    rng = np.random.default_rng(2000 + c.N + c.T + c.J)
    X, W = _covs(rng, c.N, c.T, c.J, c.Ks, c.Ko)
    D = c.Ks + c.Ko + 6
    th = _theta(rng, c.n, D, c.Ks, c.Ko)
    th[:, -4:] = (np.array([-2.0, math.log(4.0), math.log(1.5), math.log(0.7)]) + rng.uniform(-0.2, 0.2, size=(c.n, 4))).astype(np.float32)
    sc = rng.normal(size=(c.N, c.T, c.J)) * 2.0
    sc[rng.uniform(size=sc.shape) < 0.25] = np.nan
    return dict(X=X, W=W, th=th, lay=None, scores=sc.astype(np.float32))


def _score_parameters(ex):
    return ex[:, 0], ex[:, 0] + np.exp(ex[:, 1]), np.exp(ex[:, 2]), np.exp(ex[:, 3])


def _ref_scores(c, d, sign):
    eta, S_eta, nu, S_nu = _predictors(d["X"], d["W"], d["th"], None)
    mu0, mu1, sg0, sg1 = (a[:, None, None] for a in _score_parameters(_f64(d["th"])[:, c.Ks + c.Ko + 2:]))
    shape = (c.n, c.T, c.N)
    eta3, d_eta3 = np.broadcast_to(eta[:, None, :], shape), np.broadcast_to(lin_band(S_eta, c.Ks + 1)[:, None, :], shape)
    rng = R.cells(c.seed, np.arange(c.n), c.T, c.N)
    z = _latent_threshold(eta3, d_eta3, rng, sign)
    f, s, sg = (np.empty((c.n, c.J, c.T, c.N)) for _ in range(3))
    for j in range(c.J):
        x, dx = nu[:, j], lin_band(S_nu[:, j], c.Ko + 2)
        f[:, j] = rng.uniform() < z * (_sig(x) + sign * sigmoid_band(x, dx))
        g = R.normal(rng)
        s[:, j] = np.where(f[:, j] > 0, mu1 + sg1 * g, mu0 + sg0 * g)
        sg[:, j] = np.where(f[:, j] > 0, sg1, sg0)
    return dict(latent=z, f=f.astype(np.int64)), rng.taken, dict(s=s, sigma=sg)


def _handle_scores(c, d, blank=True):
    from biolith_amd.engine import OccuDataset

    obs = np.full((1, c.N, c.T, c.J), np.nan, dtype=np.float32) if blank else d["scores"][None]
    return OccuDataset(d["X"], d["W"], obs, model="occu_cs")


def _device_scores(c, d):
    ds = _handle_scores(c, d)
    z, f, s = ds.predictive_scores(d["th"], seed=c.seed)
    # tier 1 on top of the band: z and f are drawn against ``deterministic``'s float32 sites (z p_j, as occu states it), no cell left out
    psi, p = ds.deterministic(d["th"], psi=True, prob_detection=True)
    rng = R.cells(c.seed, np.arange(c.n), c.T, c.N)
    zr = rng.uniform() < psi
    assert np.array_equal(z, zr), "occu_cs z"
    for j in range(c.J):
        assert np.array_equal(f[:, j], rng.uniform() < zr * p[:, j].astype(np.float64)), ("occu_cs f", j)
        rng.uniform(), rng.uniform()                                               # the score's radius and angle
    ds.close()
    return dict(latent=z, f=f, s=s)


# ------------------------------------------------------------------------------------------------ bl_predict_comb (occu_comb) ----
def _make_comb(c):
    o = c.opt
    rng = np.random.default_rng(3000 + c.N + o["Jpc"] * 5 + o["Jaru"] * 7 + o["Js"])
    X = rng.normal(size=(c.N, c.Ks)).astype(np.float32)
    Wp = rng.normal(size=(c.N, c.T, o["Jpc"], c.Ko)).astype(np.float32)
    Wa = rng.normal(size=(c.N, c.T, o["Jaru"], o["Ka"])).astype(np.float32)
    D = c.Ks + c.Ko + o["Ka"] + 9
    th = rng.uniform(-0.7, 0.7, size=(c.n, D))
    th[:, -6:] = np.array([-1.5, -1.0, -3.0, math.log(5.0), math.log(2.0), math.log(0.8)]) + rng.uniform(-0.2, 0.2, size=(c.n, 6))
    Yp = (rng.uniform(size=(1, c.N, c.T, o["Jpc"])) < 0.3).astype(np.float32)
    Ya = (rng.uniform(size=(1, c.N, c.T, o["Jaru"])) < 0.3).astype(np.float32)
    Sc = (rng.normal(size=(1, c.N, c.T, o["Js"])) * 3.0).astype(np.float32)
    for a in (Yp, Ya, Sc):
        a[rng.uniform(size=a.shape) < 0.3] = np.nan
    return dict(X=X, Wp=Wp, Wa=Wa, th=th.astype(np.float32), Yp=Yp, Ya=Ya, Sc=Sc)


def _ref_comb(c, d, sign):
    o = c.opt
    eta, S_eta, nup, S_nup = _predictors(d["X"], d["Wp"], d["th"], None)
    _, _, nua, S_nua = _predictors(d["X"], d["Wa"], d["th"], None, al0=c.Ks + c.Ko + 2)
    ex = _f64(d["th"])[:, c.Ks + c.Ko + o["Ka"] + 3:]
    fc, fu = (_sig(ex[:, k])[:, None, None] for k in (0, 1))
    bfc, bfu = (sigmoid_band(ex[:, k], 0.0)[:, None, None] for k in (0, 1))
    mu0, mu1, sg0, sg1 = (a[:, None, None] for a in _score_parameters(ex[:, 2:]))
    shape = (c.n, c.T, c.N)
    eta3, d_eta3 = np.broadcast_to(eta[:, None, :], shape), np.broadcast_to(lin_band(S_eta, c.Ks + 1)[:, None, :], shape)
    rng = R.cells(c.seed, np.arange(c.n), c.T, c.N)
    z = _latent_threshold(eta3, d_eta3, rng, sign)
    ypc, yaru = np.empty((c.n, o["Jpc"]) + shape[1:], dtype=np.int64), np.empty((c.n, o["Jaru"]) + shape[1:], dtype=np.int64)
    s = np.empty((c.n, o["Js"]) + shape[1:])
    for j in range(o["Jpc"]):
        x, dx = nup[:, j], lin_band(S_nup[:, j], c.Ko + 1)
        ypc[:, j] = rng.uniform() < z * (_sig(x) + sign * sigmoid_band(x, dx))
    for j in range(o["Jaru"]):
        x, dx = nua[:, j], lin_band(S_nua[:, j], o["Ka"] + 1)
        pd = 1.0 - (1.0 - z * _sig(x)) * (1.0 - fc) * (1.0 - np.where(z > 0, 0.0, fu))
        yaru[:, j] = rng.uniform() < pd + sign * (z * sigmoid_band(x, dx) + bfc + bfu + 6 * U)
    for j in range(o["Js"]):
        g = R.normal(rng)
        s[:, j] = np.where(z > 0, mu1 + sg1 * g, mu0 + sg0 * g)
    sigma = np.broadcast_to(np.where(z > 0, sg1, sg0)[:, None], s.shape)
    return dict(z=z, y_pc=ypc, y_aru=yaru), rng.taken, dict(s=s, sigma=sigma)


def _handle_comb(c, d):
    from biolith_amd.engine import OccuDataset

    return OccuDataset(d["X"], d["Wp"], d["Yp"], model="occu_comb", ARU_obs_covs=d["Wa"], ARU_obs=d["Ya"], scores_obs=d["Sc"])


def _device_comb(c, d):
    ds = _handle_comb(c, d)
    th = d["th"]
    z, ypc, yaru, s = ds.predictive_comb(th, seed=c.seed)
    # every subset of the four outputs gives the bytes of the full call
    for want in itertools.product((False, True), repeat=4):
        if not any(want) or all(want):
            continue
        part = ds.predictive_comb(th, seed=c.seed, z=want[0], y_pc=want[1], y_aru=want[2], scores=want[3])
        for w, a, full in zip(want, part, (z, ypc, yaru, s)):
            assert (a is None) if not w else np.array_equal(a, full), want
    # tier 1: z and y_pc against deterministic_comb's float32 sites, no cell left out
    psi, ppc, _ = ds.deterministic_comb(th)
    rng = R.cells(c.seed, np.arange(c.n), c.T, c.N)
    zr = rng.uniform() < psi
    assert np.array_equal(z, zr), "occu_comb z"
    for j in range(c.opt["Jpc"]):
        assert np.array_equal(ypc[:, j], rng.uniform() < zr * ppc[:, j].astype(np.float64)), ("occu_comb y_pc", j)
    # tier 1: the conditional occupancy of the same handle (site_posterior serves occu_comb)
    _, q, zc = ds.site_posterior(th, seed=c.seed)
    assert np.array_equal(zc, R.cells(c.seed, np.arange(c.n), c.T, c.N).uniform() < q), "occu_comb site_posterior z"
    assert np.array_equal(ds.site_posterior(th, seed=c.seed, log_lik=False, z_prob=False)[2], zc)
    ds.close()
    return dict(z=z, y_pc=ypc, y_aru=yaru, s=s)


# ---------------------------------------------------------------------------------------------- the conditional posteriors ----
def _observations(rng, N, T, J, kind, K=0):
    if kind == "binary":
        Y = (rng.uniform(size=(N, T, J)) < 0.35 * (rng.uniform(size=(N, T, 1)) < 0.6)).astype(np.float64)
    else:
        Y = rng.poisson(rng.uniform(0.0, 2.5 if K == 0 else min(K, 3) * 0.6, size=(N, T, J)) * (rng.uniform(size=(N, T, 1)) < 0.7)).astype(np.float64)
        if K:
            Y = np.minimum(Y, K)
    Y[rng.uniform(size=Y.shape) < 0.25] = np.nan
    if N > 2:
        Y[1] = np.nan          # a site without any observation: the conditional is the prior
    return Y.astype(np.float32)


def _make_abundance(c):
    rng, X, W, lay, th = _setup_plain(c)
    o = c.opt
    th[:, 0] += 0.3
    Y = _observations(rng, c.N, c.T, c.J, "binary" if o["model"] == "occu_rn" else "count", o["K"])
    return dict(X=X, W=W, lay=lay, th=th, Y=Y)


def _ref_abundance(c, d, sign):
    o = c.opt
    u = R.cells(c.seed, np.arange(c.n), c.T, c.N)
    u0 = u.uniform()
    out = np.empty((c.n, c.T, c.N), dtype=np.int64)
    for b in range(c.n):
        th = _f64(d["th"][b])
        if o["model"] == "occu_rn":
            cl = A.rn_cells(d["X"], d["W"], d["Y"], th, o["K"], fp=o.get("fp_mode") is not None, site_re=o.get("site_re", False), obs_re=o.get("obs_re", False))
        else:
            cl = A.nmix_cells(d["X"], d["W"], d["Y"], th, o["K"], site_re=o.get("site_re", False), obs_re=o.get("obs_re", False))
        cdf = np.cumsum(cl["pmf"], axis=-1)
        band = 0.5 * A.bounds(cl, RTOL_CONDITIONAL)[0] + 2 * U          # d cdf_n / d l_m sums to 2 cdf (1 - cdf) <= 1/2
        out[b] = np.minimum((u0[b][..., None] >= cdf + sign * band[..., None]).sum(-1), o["K"])
    return dict(n_draw=out), u.taken, {}


def _device_abundance(c, d):
    ds = _handle_predict(c, d)
    full = ds.abundance_posterior(d["th"], seed=c.seed)
    only = ds.abundance_posterior(d["th"], seed=c.seed, log_lik=False, n_mean=False, occ_prob=False)
    assert np.array_equal(only[3], full[3])
    ds.close()
    return dict(n_draw=full[3])


def _make_score_post(c):
    return _make_scores(c)


def _ref_score_post(c, d, sign, z_prob=None):
    """z ~ [u0 < z_prob] (the device's own float32 z_prob where given: tier 1; else the restatement's q -/+ its allowance), then per
    visit f_j = z [u_j < r_j], r_j = sigmoid((log p_j + n1_j) - (log(1 - p_j) + n0_j)), the detection probability itself where masked."""
    X, W, Sc = d["X"], d["W"], d["scores"]
    rng = R.cells(c.seed, np.arange(c.n), c.T, c.N)
    u0 = rng.uniform()
    z = np.empty((c.n, c.T, c.N), dtype=bool)
    f = np.empty((c.n, c.J, c.T, c.N), dtype=np.int64)
    _, _, nu, S_nu = _predictors(X, W, d["th"], None)
    s = np.nan_to_num(_f64(Sc)).transpose(2, 1, 0)[None]                            # (1, J, T, N)
    m = np.isfinite(_f64(Sc)).transpose(2, 1, 0)[None]
    mu0, mu1, sg0, sg1 = (a[:, None, None, None] for a in _score_parameters(_f64(d["th"])[:, c.Ks + c.Ko + 2:]))
    lp, l1p = -np.logaddexp(0.0, -nu), -np.logaddexp(0.0, nu)
    n0 = -0.5 * ((s - mu0) / sg0) ** 2 - np.log(sg0) - SR.HL2PI
    n1 = -0.5 * ((s - mu1) / sg1) ** 2 - np.log(sg1) - SR.HL2PI
    r = np.where(m, _sig((lp + n1) - (l1p + n0)), _sig(nu))
    scale = np.where(m, np.abs(lp) + np.abs(n1) + np.abs(l1p) + np.abs(n0), 0.0)
    br = np.where(m, 0.25 * (RTOL_CONDITIONAL * scale + lin_band(S_nu, c.Ko + 2)) + 2 * U, sigmoid_band(nu, lin_band(S_nu, c.Ko + 2)))
    for b in range(c.n):
        if z_prob is None:
            cl = SR.cs_cells(X, W, Sc, _f64(d["th"][b]))
            z[b] = u0[b] < cl["q"] + sign * SR.bounds(cl, RTOL_CONDITIONAL)[1]
        else:
            z[b] = u0[b] < z_prob[b]
    for j in range(c.J):
        f[:, j] = z & (rng.uniform() < r[:, j] + sign * br[:, j])
    return dict(z=z.astype(np.int64), f=f), rng.taken, {}


def _device_score_post(c, d):
    ds = _handle_scores(c, d, blank=False)
    ll, q, z, fp, f = ds.score_posterior(d["th"], seed=c.seed)
    short = ds.score_posterior(d["th"], seed=c.seed, visits=False)
    assert short[3] is None and short[4] is None and np.array_equal(short[2], z) and np.array_equal(short[1], q)
    ds.close()
    return dict(z=z, f=f, z_prob=q)


def _make_count_post(c):
    rng, X, W, lay, th = _setup_plain(c)
    th[:, c.Ks + 1] += 0.3
    Y = _observations(rng, c.N, c.T, c.J, "count")
    dur = rng.uniform(0.5, 3.0, size=(c.N, c.T, c.J)).astype(np.float32)
    return dict(X=X, W=W, lay=lay, th=th, Y=Y, dur=dur)


def _ref_count_post(c, d, sign, z_prob=None):
    """z ~ [u0 < z_prob], then per visit true_count_j = z Binomial(y_j, rho_j) in constant mode (y_j uniforms, whatever z is), z y_j
    in the other modes (no uniform)."""
    o = c.opt
    fpm = o.get("fp_mode")
    rng = R.cells(c.seed, np.arange(c.n), c.T, c.N)
    u0 = rng.uniform()
    z = np.empty((c.n, c.T, c.N), dtype=bool)
    rho, brho = np.empty((c.n, c.J, c.T, c.N)), np.empty((c.n, c.J, c.T, c.N))
    _, _, nu, S_nu = _predictors(d["X"], d["W"], d["th"], d["lay"])
    for b in range(c.n):
        th = _f64(d["th"][b])
        cl = CR.cop_cells(d["X"], d["W"], d["Y"], d["dur"], th, fp_mode=fpm, site_re=o.get("site_re", False), obs_re=o.get("obs_re", False))
        z[b] = u0[b] < (cl["q"] + sign * CR.bounds(cl, RTOL_CONDITIONAL)[1] if z_prob is None else z_prob[b])
        rho[b], y = cl["rho"], cl["y"]
        # rho = lambda rcp(lambda + f) = sigmoid(nu - phi): the two exponentials' relative errors and nu's own, a quarter, + 8 u
        brho[b] = 0.25 * (lin_band(S_nu[b], c.Ko + 2) + (cl["S_v"] + 8.0) * 2 * U) + 8 * U
    y = y.astype(np.int64)                                                           # (J, T, N): the data, the same for every draw
    t = np.empty((c.n, c.J, c.T, c.N), dtype=np.int64)
    for j in range(c.J):
        yj = np.broadcast_to(y[j][None], (c.n, c.T, c.N))
        t[:, j] = z * (R.binomial(rng, yj, rho[:, j] + sign * brho[:, j]) if fpm == "constant" else yj)
    return dict(z=z.astype(np.int64), true_count=t), rng.taken, {}


def _device_count_post(c, d):
    ds = _handle_predict(c, d)
    ll, q, z, tm, tc = ds.count_posterior(d["th"], seed=c.seed)
    short = ds.count_posterior(d["th"], seed=c.seed, visits=False)
    assert short[3] is None and short[4] is None and np.array_equal(short[2], z) and np.array_equal(short[1], q)
    ds.close()
    return dict(z=z, true_count=tc, z_prob=q)


def _make_path(c):
    rng = np.random.default_rng(5000 + c.N + c.T)
    X, W = _covs(rng, c.N, c.T, c.J, c.Ks, c.Ko)
    D = 3 * (c.Ks + 1) + c.Ko + 1
    th = rng.uniform(-0.7, 0.7, size=(c.n, D))
    th[:, c.Ks + 1] -= 1.2          # colonisation and extinction around 0.2
    th[:, 2 * (c.Ks + 1)] -= 1.2
    Y = _observations(rng, c.N, c.T, c.J, "binary")
    return dict(X=X, W=W, th=th.astype(np.float32), Y=Y)


def _ref_path(c, d, sign, z_prob=None):
    """One generator per (n, t, i), its first uniform: z_T-1 ~ [u < z_prob[T-1]], then backwards z_t ~ [u < b_1 or b_0 given z_t+1]."""
    rng = R.cells(c.seed, np.arange(c.n), c.T, c.N)
    u = rng.uniform()
    z = np.empty((c.n, c.T, c.N), dtype=bool)
    for b in range(c.n):
        cl = DP.dyn_paths(d["X"], d["W"], d["Y"], _f64(d["th"][b]))
        band = DP.bounds(cl, DP.RTOL)[1]
        last = cl["q"][c.T - 1] + sign * band if z_prob is None else z_prob[b, c.T - 1]
        z[b, c.T - 1] = u[b, c.T - 1] < last
        for t in range(c.T - 2, -1, -1):
            z[b, t] = u[b, t] < np.where(z[b, t + 1], cl["bk1"][t], cl["bk0"][t]) + sign * band
    return dict(z=z.astype(np.int64)), rng.taken, dict(path=True)


def _device_path(c, d):
    from biolith_amd.engine import OccuDataset

    ds = OccuDataset(d["X"], d["W"], d["Y"][None], model="occu_dyn")
    full = ds.path_posterior(d["th"], seed=c.seed)
    only = ds.path_posterior(d["th"], seed=c.seed, log_lik=False, col_prob=False, ext_prob=False)
    assert np.array_equal(only[4], full[4]) and np.array_equal(only[1], full[1])
    ds.close()
    return dict(z=full[4], z_prob=full[1])


FAMILIES = {
    "predict": (_make_predict, _ref_predict, _device_predict),
    "counts": (_make_counts, _ref_counts, _device_predict),
    "scores": (_make_scores, _ref_scores, _device_scores),
    "comb": (_make_comb, _ref_comb, _device_comb),
    "abundance_post": (_make_abundance, _ref_abundance, _device_abundance),
    "score_post": (_make_score_post, _ref_score_post, _device_score_post),
    "count_post": (_make_count_post, _ref_count_post, _device_count_post),
    "path_post": (_make_path, _ref_path, _device_path),
}

S32, S64 = 2 ** 32, 2 ** 64 - 1
CASES = [
    # bl_predict: occu_fp in both modes, every random-effects kind, Royle-Nichols (max_abundance 1, 6, 127; a false-positive rate; effects)
    Case("occu_fp-constant", "predict", 63, 3, 4, 2, 2, 3, S32, model="occu_fp", fp_mode="constant"),
    Case("occu_fp-unoccupied", "predict", 65, 1, 4, 5, 0, 3, S64, model="occu_fp", fp_mode="unoccupied"),
    Case("occu_re-site", "predict", 63, 3, 4, 2, 2, 3, 0, model="occu_re", site_re=True),
    Case("occu_re-obs", "predict", 65, 3, 4, 0, 5, 3, S32, model="occu_re", obs_re=True),
    Case("occu_re-both-fp-constant", "predict", 257, 3, 4, 2, 2, 3, S64, model="occu_re", site_re=True, obs_re=True, fp_mode="constant"),
    Case("occu_re-obs-fp-unoccupied", "predict", 1, 3, 4, 2, 2, 3, 0, model="occu_re", obs_re=True, fp_mode="unoccupied"),
    Case("occu_rn-K1", "predict", 1, 1, 1, 0, 0, 3, 0, model="occu_rn", K=1),
    Case("occu_rn-K6", "predict", 63, 3, 4, 2, 5, 3, S32, model="occu_rn", K=6),
    Case("occu_rn-K127", "predict", 257, 1, 4, 5, 2, 3, S64, model="occu_rn", K=127),
    Case("occu_rn-fp", "predict", 65, 3, 4, 2, 2, 3, S32, model="occu_rn", K=6, fp_mode="constant"),
    Case("occu_rn-effects", "predict", 65, 3, 4, 2, 2, 3, 0, model="occu_rn", K=6, site_re=True, obs_re=True),
    Case("occu_rn-grid-rows", "predict", 5, 3, 4, 2, 2, 1030, S32, model="occu_rn", K=6),
    # bl_predict_counts
    Case("nmixture-K1", "counts", 1, 3, 4, 2, 0, 3, 0, model="nmixture", K=1),
    Case("nmixture-K6", "counts", 63, 3, 4, 2, 2, 3, S32, model="nmixture", K=6),
    Case("nmixture-K127", "counts", 65, 1, 4, 5, 5, 3, S64, model="nmixture", K=127),
    Case("nmixture-effects", "counts", 257, 3, 1, 2, 2, 3, S32, model="nmixture", K=6, site_re=True, obs_re=True),
    Case("nmixture-grid-rows", "counts", 5, 3, 4, 2, 2, 1030, 0, model="nmixture", K=6),
    Case("occu_cop", "counts", 63, 3, 4, 2, 2, 3, S32, model="occu_cop"),
    Case("occu_cop-constant", "counts", 65, 1, 4, 5, 0, 3, S64, model="occu_cop", fp_mode="constant"),
    Case("occu_cop-unoccupied", "counts", 257, 3, 1, 0, 2, 3, 0, model="occu_cop", fp_mode="unoccupied"),
    Case("occu_cop-effects", "counts", 65, 3, 4, 2, 2, 3, S32, model="occu_cop", site_re=True, obs_re=True, fp_mode="constant"),
    # bl_predict_scores, bl_predict_comb (unequal visit counts, one of them 0)
    Case("occu_cs", "scores", 63, 3, 4, 2, 5, 3, S32),
    Case("occu_cs-one-visit", "scores", 257, 1, 1, 0, 0, 3, S64),
    Case("occu_comb-2-3-1", "comb", 63, 3, 2, 2, 2, 3, S32, Jpc=2, Jaru=3, Js=1, Ka=1),
    Case("occu_comb-0-4-2", "comb", 65, 1, 0, 5, 0, 3, S64, Jpc=0, Jaru=4, Js=2, Ka=5),
    Case("occu_comb-3-0-0", "comb", 257, 3, 3, 0, 2, 1, 0, Jpc=3, Jaru=0, Js=0, Ka=0),
    Case("occu_comb-1-1-3", "comb", 1, 3, 1, 2, 2, 3, 0, Jpc=1, Jaru=1, Js=3, Ka=2),
    # the conditional posteriors
    Case("abundance-occu_rn", "abundance_post", 63, 3, 4, 2, 2, 3, S32, model="occu_rn", K=6),
    Case("abundance-occu_rn-fp-effects", "abundance_post", 65, 1, 4, 2, 2, 3, S64, model="occu_rn", K=6, fp_mode="constant", site_re=True, obs_re=True),
    Case("abundance-nmixture", "abundance_post", 257, 3, 1, 2, 2, 3, 0, model="nmixture", K=6),
    Case("abundance-nmixture-K127", "abundance_post", 65, 3, 4, 0, 5, 3, S32, model="nmixture", K=127, obs_re=True),
    Case("score_posterior", "score_post", 63, 3, 4, 2, 2, 3, S32),
    Case("score_posterior-one-visit", "score_post", 257, 1, 1, 5, 0, 3, S64),
    Case("count_posterior-constant", "count_post", 63, 3, 4, 2, 2, 3, S32, model="occu_cop", fp_mode="constant"),
    Case("count_posterior-unoccupied", "count_post", 65, 1, 4, 2, 2, 3, S64, model="occu_cop", fp_mode="unoccupied"),
    Case("count_posterior-none", "count_post", 257, 3, 1, 0, 2, 3, 0, model="occu_cop"),
    Case("count_posterior-constant-effects", "count_post", 65, 3, 4, 2, 2, 3, 0, model="occu_cop", fp_mode="constant", site_re=True, obs_re=True),
    Case("path_posterior-T3", "path_post", 63, 3, 4, 2, 2, 3, S32),
    Case("path_posterior-T1", "path_post", 257, 1, 4, 2, 2, 3, S64),
    Case("path_posterior-grid-rows", "path_post", 5, 3, 1, 0, 0, 1030, 0),
]


def _reduce(eq, path):
    if eq.ndim == 4:
        eq = eq.all(axis=1)
    if path:                      # path_posterior: the path of a site is one draw across its periods
        eq = np.broadcast_to(eq.all(axis=1, keepdims=True), eq.shape)
    return eq


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(the case, its data, the reference's outputs, the decided cells (n, T, N), the float outputs' reference)."""
    c = next(k for k in CASES if k.name == name)
    make, ref, _ = FAMILIES[c.family]
    d = make(c)
    lo, t_lo, aux = ref(c, d, -1)
    hi, t_hi, _ = ref(c, d, +1)
    path = bool(aux.get("path"))
    dec = _reduce(t_lo == t_hi, path)
    for k in lo:
        dec = dec & _reduce(lo[k] == hi[k], path)
    for a in list(lo.values()) + [dec]:
        a.setflags(write=False)
    return c, d, lo, dec, aux


def _share(dec):
    return 1.0 - float(dec.mean())


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_undecided_share(name):
    """From the reference alone (no GPU): the bands leave at most 1e-3 of a case's cells undecided."""
    c, _, _, dec, aux = _reference(name)
    print(f"[{name}] undecided cells: {_share(dec):.2e} of {dec.size}")
    assert _share(dec) <= CAP, (name, _share(dec))
    for what, ok in aux.get("checks", []):   # the case reaches the edge it was built for
        assert ok, (name, what)


def _expand(dec, a):
    return np.broadcast_to(dec[:, None], a.shape) if a.ndim == 4 else dec


def _compare_scores(name, got, aux, dec):
    m = _expand(dec, got)
    err = np.abs(got.astype(np.float64) - aux["s"]) / aux["sigma"]
    worst = float(err[m].max()) if m.any() else 0.0
    print(f"[{name}] scores: max |s - s_ref| / sigma on decided cells = {worst:.3e} (tolerance {SCORE_TOL:.1e})")
    assert worst <= SCORE_TOL, (name, worst)


@gpu
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_decided_cells_equal_the_device(name):
    c, d, want, dec, aux = _reference(name)
    print(f"[{name}] undecided cells: {_share(dec):.2e} of {dec.size}")
    assert _share(dec) <= CAP
    got = FAMILIES[c.family][2](c, d)
    if "z_prob" in got:   # tier 1 first: z against the float32 z_prob the kernel returned, no cell left out
        q = got["z_prob"]
        if c.family == "path_post":
            u = R.cells(c.seed, np.arange(c.n), c.T, c.N).uniform()
            assert np.array_equal(got["z"][:, c.T - 1], u[:, c.T - 1] < q[:, c.T - 1]), (name, "z of the last period")
        else:
            assert np.array_equal(got["z"], R.cells(c.seed, np.arange(c.n), c.T, c.N).uniform() < q), (name, "z")
        # ... and the visit-level draws follow the z the device drew: the reference again, from the device's z_prob
        want = FAMILIES[c.family][1](c, d, -1, z_prob=q)[0]
        hi = FAMILIES[c.family][1](c, d, +1, z_prob=q)[0]
        dec = np.ones_like(dec)
        for k in want:
            dec = dec & _reduce(want[k] == hi[k], bool(aux.get("path")))
        print(f"[{name}] undecided cells given the device's z_prob: {_share(dec):.2e}")
        assert _share(dec) <= CAP
    for k, ref in want.items():
        m = _expand(dec, ref)
        assert got[k].shape == ref.shape, (name, k, got[k].shape, ref.shape)
        bad = (got[k].astype(np.int64) != ref) & m
        assert not bad.any(), (name, k, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    if "s" in aux:
        _compare_scores(name, got["s"], aux, dec)


# ------------------------------------------------------------------------------------------------- tier 1: occu, cell by cell ----
def _occu_case(N, T, J, Ks, Ko, n, seed):
    rng = np.random.default_rng(N * 31 + T * 7 + J + Ks + Ko)
    X, W = _covs(rng, N, T, J, Ks, Ko)
    return X, W, _theta(rng, n, Ks + Ko + 2, Ks, Ko)


def _occu_reference(ds, th, seed, draws=None, sites=None):
    """z, y of bl_predict for an occu handle from ``deterministic``'s float32 sites: z = [u0 < psi], y_j = [u_1+j < z p_j]."""
    psi, p = ds.deterministic(th, psi=True, prob_detection=True)
    draws = np.arange(th.shape[0]) if draws is None else np.asarray(draws)
    sites = np.arange(ds.N) if sites is None else np.asarray(sites)
    psi, p = psi[draws][:, :, sites].astype(np.float64), p[draws][:, :, :, sites].astype(np.float64)
    rng = R.cells(seed, draws, ds.T, ds.N, sites)
    z = rng.uniform() < psi
    y = np.stack([rng.uniform() < z * p[:, j] for j in range(ds.J)], axis=1) if ds.J else np.empty((len(draws), 0) + z.shape[1:], dtype=bool)
    return z, y


@gpu
@pytest.mark.parametrize("N,T,J,Ks,Ko,n,seed", [(1, 1, 1, 0, 0, 3, 0), (63, 3, 4, 2, 5, 3, S32), (65, 1, 4, 5, 2, 1, S64),
                                               (257, 3, 1, 2, 0, 3, 7 + 5 * S32), (5, 3, 4, 2, 2, 1030, S32)])
def test_occu_exact(N, T, J, Ks, Ko, n, seed):
    from biolith_amd.engine import OccuDataset

    X, W, th = _occu_case(N, T, J, Ks, Ko, n, seed)
    ds = OccuDataset(X, W, np.full((1, N, T, J), np.nan, dtype=np.float32))
    z, y = ds.predictive(th, seed=seed)
    zr, yr = _occu_reference(ds, th, seed)
    assert np.array_equal(z, zr), ("z", int((z != zr).sum()))
    assert np.array_equal(y, yr), ("y", int((y != yr).sum()))
    assert np.array_equal(ds.predictive(th, seed=seed, latent=False)[1], y) and np.array_equal(ds.predictive(th, seed=seed, y=False)[0], z)
    ds.close()


@gpu
def test_a_tie_is_not_a_success():
    """``u < p`` is strict, and a tie cannot be left to chance (2^-24 a cell): the draws are built so that the threshold EQUALS the
    cell's uniform.  One site, one visit, no covariates: psi is a function of the draw's intercept alone, the uniforms of cell n are
    known beforehand, and for u in [0.5, 0.73) an ulp of the intercept moves the float32 sigmoid by less than the uniforms' grid, so a
    few neighbouring intercepts are tried until ``deterministic`` returns u itself.  Even draws tie z, odd draws (psi = 1) tie y."""
    from biolith_amd.engine import OccuDataset

    n, seed = 600, S32 + 1
    ds = OccuDataset(np.zeros((1, 0), np.float32), np.zeros((1, 1, 1, 0), np.float32), np.full((1, 1, 1, 1), np.nan, np.float32))
    rng = R.cells(seed, np.arange(n), 1, 1)
    u0, u1 = rng.uniform()[:, 0, 0], rng.uniform()[:, 0, 0]
    even = np.arange(n) % 2 == 0
    tgt, col = np.where(even, u0, u1), np.where(even, 0, 1)
    cand = (tgt > 0.51) & (tgt < 0.73)
    x32 = np.log(np.where(cand, tgt, 0.6) / (1.0 - np.where(cand, tgt, 0.6))).astype(np.float32)
    th = np.zeros((n, 2), dtype=np.float32)
    th[~even, 0] = 20.0                                                               # psi = 1: z = 1, the visit decides
    found = np.zeros(n, dtype=bool)
    for k in (0, 1, -1, 2, -2, 3, -3, 4, -4):
        trial = th.copy()
        trial[np.arange(n), col] = np.where(found, th[np.arange(n), col], (x32.view(np.int32) + k).view(np.float32))
        psi, p = ds.deterministic(trial, psi=True, prob_detection=True)
        val = np.where(even, psi[:, 0, 0], p[:, 0, 0, 0]).astype(np.float64)
        hit = cand & ~found & (val == tgt)
        th[hit] = trial[hit]
        found |= hit
    th[~found] = np.where(even[~found, None], np.float32([0.3, -0.2]), np.float32([20.0, 0.1]))
    assert (found & even).sum() >= 10 and (found & ~even).sum() >= 10, (int((found & even).sum()), int((found & ~even).sum()))
    z, y = ds.predictive(th, seed=seed)
    zr, yr = _occu_reference(ds, th, seed)
    assert np.array_equal(z, zr) and np.array_equal(y, yr)
    assert not z[found & even].any() and z[~even].all() and not y[found & ~even].any()
    ds.close()


@gpu
def test_seeds_that_differ_above_bit_32():
    """predict() keys species sp with random_seed + (sp << 32): the upper half of the seed must reach the generator."""
    from biolith_amd.engine import OccuDataset

    N, T, J = 65, 3, 4
    X, W, th = _occu_case(N, T, J, 2, 2, 3, 0)
    ds = OccuDataset(X, W, np.full((1, N, T, J), np.nan, dtype=np.float32))
    out = []
    for seed in (11, 11 + S32, 11 + (S32 << 31)):
        z, y = ds.predictive(th, seed=seed)
        zr, yr = _occu_reference(ds, th, seed)
        assert np.array_equal(z, zr) and np.array_equal(y, yr), seed
        out.append((z, y))
    assert not np.array_equal(out[0][1], out[1][1]) and not np.array_equal(out[0][1], out[2][1]) and not np.array_equal(out[1][1], out[2][1])
    ds.close()


@gpu
@pytest.mark.parametrize("kind", ["occu", "occu_fp-constant", "occu_fp-unoccupied", "occu_re", "occu_re-fp"])
def test_site_posterior_exact(kind):
    """z = [u0 < z_prob] with the z_prob the kernel returned, in every cell; z alone gives the same bytes."""
    from biolith_amd.engine import OccuDataset

    N, T, J, Ks, Ko, n = {"occu": (257, 3, 4, 2, 5), "occu_re": (65, 3, 4, 2, 2)}.get(kind, (63, 3, 4, 5, 2)) + (3,)
    rng = np.random.default_rng(len(kind))
    X, W = _covs(rng, N, T, J, Ks, Ko)
    Y = _observations(rng, N, T, J, "binary")[None]
    kw = {"occu": {}, "occu_fp-constant": dict(model="occu_fp", fp_mode="constant"), "occu_fp-unoccupied": dict(model="occu_fp", fp_mode="unoccupied"),
          "occu_re": dict(model="occu_re", site_random_effects=True, obs_random_effects=True),
          "occu_re-fp": dict(model="occu_re", site_random_effects=True, re_fp_mode="constant")}[kind]
    ds = OccuDataset(X, W, Y, **kw)
    th = _theta(rng, n, ds.D, Ks, Ko)
    for seed in (0, S32, S64):
        _, q, z = ds.site_posterior(th, seed=seed)
        assert np.array_equal(z, R.cells(seed, np.arange(n), T, N).uniform() < q), (kind, seed)
        assert np.array_equal(ds.site_posterior(th, seed=seed, log_lik=False, z_prob=False)[2], z)
    assert 0.02 < z.mean() < 0.98
    ds.close()


@gpu
def test_site_posterior_beyond_the_grid_rows():
    from biolith_amd.engine import OccuDataset

    N, T, J, n = 5, 3, 4, 1030
    rng = np.random.default_rng(8)
    X, W = _covs(rng, N, T, J, 2, 2)
    ds = OccuDataset(X, W, _observations(rng, N, T, J, "binary")[None])
    th = _theta(rng, n, ds.D, 2, 2)
    _, q, z = ds.site_posterior(th, seed=S32)
    assert np.array_equal(z, R.cells(S32, np.arange(n), T, N).uniform() < q)
    ds.close()


@gpu
def test_predict_chunk_boundary():
    """bl_predict across its 256 MB chunks: N = 20000, J = 4, n = 3400, y only (272 MB; one chunk holds 3355 draws).  The reference at
    the draws on both sides of the boundary and at both ends, on 2000 sampled sites: the absolute draw index keys the generator."""
    from biolith_amd.engine import OccuDataset

    N, T, J, n = 20000, 1, 4, 3400
    rng = np.random.default_rng(20)
    X, W = _covs(rng, N, T, J, 2, 2)
    th = _theta(rng, n, 6, 2, 2)
    ds = OccuDataset(X, W, np.full((1, N, T, J), np.nan, dtype=np.float32))
    assert (256 << 20) // (N * T * J) == 3355
    _, y = ds.predictive(th, seed=S32 + 3, latent=False)
    draws, sites = np.array([0, 3354, 3355, 3399]), np.sort(rng.choice(N, size=2000, replace=False))
    _, yr = _occu_reference_rows(ds, th, S32 + 3, draws, sites)
    got = y[draws][:, :, :, sites]
    assert np.array_equal(got, yr), int((got != yr).sum())
    ds.close()


def _occu_reference_rows(ds, th, seed, draws, sites):
    """``_occu_reference`` for a few draws of a long matrix: ``deterministic`` is given those rows only (its sites do not depend on the
    draw's index), the generator their absolute indices."""
    psi, p = ds.deterministic(th[draws], psi=True, prob_detection=True)
    psi, p = psi[:, :, sites].astype(np.float64), p[:, :, :, sites].astype(np.float64)
    rng = R.cells(seed, draws, ds.T, ds.N, sites)
    z = rng.uniform() < psi
    return z, np.stack([rng.uniform() < z * p[:, j] for j in range(ds.J)], axis=1)
