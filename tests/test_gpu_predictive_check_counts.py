"""predictive_check_counts on the GPU: the fused check (bl_predictive_check_counts) of occu_rn, nmixture and occu_cop against its
definition restated in float64 NumPy on predict()'s arrays for the same seed -- for every grouping and statistic and every served
handle; the geometry (one site, a tail block, more draws than grid rows, the same bytes twice, one output without the other); both
branches of the Poisson sampler, a truncation that bites, rates whose exp(-lambda) underflows; missing revisits, sites, observations
and covariates; a small real fit; the refusals at the C-ABI.

Posteriors are hand-made (random float32 coefficients behind a ``get_samples()`` stub); one fit of 60 sites, 100 + 100 draws.

The restatement here is independent of both implementations: the restricted Poisson's weights in logs (n log(lambda) - lgamma(n + 1),
the largest subtracted), where the device and ``evaluation.posterior_predictive_check_counts`` run a scaled recursion.  A sampled
false-positive rate enters E as the float32 site value the layout's transform gives the draw's coordinate (``_site_rate``).

Tolerance: the replicate is predict()'s bit for bit, so its group totals are equal integers; E has bit-equal float32 inputs.  What
remains is libm in the truncated sums (at most 128 terms, a few ulp each; in logs the argument reaches ~1500, so ~1e-13) and the order of
at most ~10^4 non-negative float64 additions: rtol 1e-9 on d_obs and d_rep, atol 0.  The p-value equals mean(d_rep > d_obs) of the
returned arrays exactly, and the host function's up to the draws with 0 < |d_rep - d_obs| <= 1e-9 max(d_rep, d_obs), of which there may
be at most n / 100."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest
from scipy.special import gammaln, xlogy

from biolith_amd import _ffi, models
from biolith_amd.engine import OccuDataset
from biolith_amd.evaluation import posterior_predictive_check_counts
from biolith_amd.models import simulate, simulate_nmixture
from biolith_amd.utils import fit, predict, predictive_check_counts

pytestmark = pytest.mark.gpu

RTOL = 1e-9
PAIRS = [(g, s) for g in ("site", "revisit") for s in ("freeman-tukey", "chi-squared")]
MODELS = ["nmixture", "occu_rn", "occu_cop"]
WORST = {"err": 0.0}   # the largest relative error any comparison of this run has seen (printed by every comparison)


class _Posterior:
    """What predict and predictive_check_counts read of a fit: ``get_samples()``."""

    def __init__(self, sites):
        self.sites = sites

    def get_samples(self):
        return self.sites


def _case(name, seed, N, T, J, n, Ks=2, Ko=2, missing=0.1, fp=None, re=False, max_abundance=None, intercept=None, hot_draw=None,
          dur_max=40.0):
    """Random data with ``missing`` of obs NaN, a hand-made posterior for it, and the model options (``session_duration`` among them).
    ``intercept``: every draw's abundance intercept; ``hot_draw``: draw 0's, on top."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    data = dict(site_covs=f32(rng.normal(size=(N, Ks))), obs_covs=f32(rng.normal(size=(N, T, J, Ko))))
    obs = rng.poisson(2.0, (1, N, T, J)).astype(np.float32)
    if name == "occu_rn":
        obs = np.minimum(obs, 1.0)
    obs[rng.random(obs.shape) < missing] = np.nan
    data["obs"] = obs
    sites = dict(beta=f32(rng.uniform(-1, 1, (n, 1, Ks + 1))), alpha=f32(rng.uniform(-1, 1, (n, 1, Ko + 1))))
    if intercept is not None:
        sites["beta"][:, :, 0] = intercept
    if hot_draw is not None:
        sites["beta"][0, :, 0] = hot_draw
    opts = {}
    if name == "occu_cop":
        opts["session_duration"] = f32(rng.uniform(0.5, dur_max, (N, T, J)))
    if max_abundance is not None:
        opts["max_abundance"] = max_abundance
    if fp:
        opts[f"false_positives_{fp}"] = True
        if name == "occu_cop":
            sites[f"rate_fp_{fp}"] = f32(rng.uniform(0.05, 0.8, n))
        else:
            sites[f"prob_fp_{fp}"] = f32(rng.uniform(0.05, 0.3, n))
    if re:
        opts.update(site_random_effects=True, obs_random_effects=True)
        first = "site_re_occ" if name == "occu_cop" else "site_re_abu"
        sites.update({"site_re_sd": f32(rng.uniform(0.3, 1.0, n)), first: f32(rng.normal(0, 0.5, (n, N, 1))),
                      "site_re_det": f32(rng.normal(0, 0.5, (n, N, 1))), "obs_re_sd": f32(rng.uniform(0.3, 1.0, n)),
                      "obs_re": f32(rng.normal(0, 0.5, (n, J, T, N, 1)))})
    return data, _Posterior(sites), opts


def _site_rate(site, transform):
    """The float32 site value of the draw's coordinate: the site -> the layout's float32 coordinate -> its float64 transform -> float32."""
    v = np.asarray(site, dtype=np.float64)
    if transform == "sigmoid":
        v = np.clip(v, 1e-300, 1 - 1e-16)
        phi = np.log(v / (1.0 - v)).astype(np.float32).astype(np.float64)
        return (1.0 / (1.0 + np.exp(-phi))).astype(np.float32)
    phi = np.log(np.maximum(v, 1e-300)).astype(np.float32).astype(np.float64)
    return np.exp(phi).astype(np.float32)


def _rates(name, sites):
    """The sampled false-positive site as E takes it, by name."""
    return {k: _site_rate(v, "exp" if name == "occu_cop" else "sigmoid") for k, v in sites.items() if k.startswith(("prob_fp_", "rate_fp_"))}


def _weights(lam, K):
    """(..., K + 1): the pmf of Poisson(lam) restricted to 0..K, through logs."""
    support = np.arange(K + 1, dtype=np.float64)
    logw = xlogy(support, lam[..., None]) - gammaln(support + 1.0)
    w = np.exp(logw - logw.max(axis=-1, keepdims=True))
    return w / w.sum(axis=-1, keepdims=True)


def _expected(name, preds, rates, dur, K):
    """E (n, J, T, N, S) float64 from predict()'s float32 sites."""
    col = (-1,) + (1,) * 4
    if name == "occu_cop":
        psi = np.asarray(preds["psi"], dtype=np.float64)[:, None]
        rate = np.asarray(preds["rate_detection"], dtype=np.float64)
        d = np.asarray(dur, dtype=np.float64).transpose(2, 1, 0)[None, ..., None]
        f_c = rates["rate_fp_constant"].astype(np.float64).reshape(col) if "rate_fp_constant" in rates else 0.0
        f_u = rates["rate_fp_unoccupied"].astype(np.float64).reshape(col) if "rate_fp_unoccupied" in rates else 0.0
        return d * (psi * rate + (1.0 - psi) * f_u + f_c)
    lam = np.asarray(preds["abundance"], dtype=np.float64)
    p = np.asarray(preds["prob_detection"], dtype=np.float64)
    w = _weights(lam, K)                                                              # (n, T, N, S, K + 1)
    if name == "nmixture":
        return (w * np.arange(K + 1)).sum(axis=-1)[:, None] * p
    f = rates["prob_fp_constant"].astype(np.float64).reshape(col) if "prob_fp_constant" in rates else 0.0
    miss = np.zeros(p.shape)
    for k in range(K + 1):
        miss += w[..., k][:, None] * (1.0 - p) ** k
    return 1.0 - (1.0 - f) * miss


def _host(name, preds, rates, obs, dur, K, group_by, statistic):
    """d_obs, d_rep (n,) by the definition, in float64 NumPy."""
    stat = {"freeman-tukey": lambda o, e: (np.sqrt(o) - np.sqrt(e)) ** 2, "chi-squared": lambda o, e: (o - e) ** 2 / (e + 1e-10)}[statistic]
    obs = np.asarray(obs, dtype=np.float64)
    y_rep = np.asarray(preds["y"], dtype=np.float64).transpose((0, 4, 3, 2, 1))
    expected = _expected(name, preds, rates, dur, K).transpose((0, 4, 3, 2, 1))
    seen = ~np.isnan(obs)[None]
    axes_obs, axes_rep = ((2, 3), (3, 4)) if group_by == "site" else ((1,), (2,))
    obs_g = np.nansum(obs, axis=axes_obs)
    rep_g = np.where(seen, y_rep, 0.0).sum(axis=axes_rep)
    exp_g = np.where(seen, expected, 0.0).sum(axis=axes_rep)
    axes = tuple(range(1, exp_g.ndim))
    return stat(obs_g[None], exp_g).sum(axis=axes), stat(rep_g, exp_g).sum(axis=axes)


def _branches(name, preds, rates, dur, K):
    """The share of cells in each branch of the kernel's arithmetic, printed with every comparison."""
    if name == "occu_cop":
        z = np.asarray(preds["z"], dtype=np.float64)[:, None]
        col = (-1,) + (1,) * 4
        f_c = rates["rate_fp_constant"].astype(np.float64).reshape(col) if "rate_fp_constant" in rates else 0.0
        f_u = rates["rate_fp_unoccupied"].astype(np.float64).reshape(col) if "rate_fp_unoccupied" in rates else 0.0
        rate = np.asarray(dur, dtype=np.float64).transpose(2, 1, 0)[None, ..., None] * (z * preds["rate_detection"] + (1 - z) * f_u + f_c)
        return f"Poisson rate 0: {np.mean(rate <= 0):.3f}, below 10 (inversion): {np.mean((rate > 0) & (rate < 10)):.3f}, from 10 (PTRS): {np.mean(rate >= 10):.3f}"
    lam = np.asarray(preds["abundance"], dtype=np.float64)
    return (f"N_i at the cap K={K}: {np.mean(np.asarray(preds['N_i']) == K):.3f}, lambda > K: {np.mean(lam > K):.3f}, "
            f"lambda > 745: {np.mean(lam > 745):.3f}")


def _compare(name, data, posterior, opts, seed=5, pairs=PAIRS):
    """The fused check against the restated definition on predict()'s arrays, same seed; returns the fused results by pair."""
    model = getattr(models, name)
    n = posterior.sites["beta"].shape[0]
    K, dur = opts.get("max_abundance", 100), opts.get("session_duration")
    preds = predict(model, posterior, **data, num_samples=n, random_seed=seed, **opts)
    rates = _rates(name, posterior.sites)
    print(f"{name}: {_branches(name, preds, rates, dur, K)}")
    out = {}
    for g, s in pairs:
        got = predictive_check_counts(model, posterior, **data, group_by=g, statistic=s, random_seed=seed, **opts)
        d_obs, d_rep = _host(name, preds, rates, data["obs"], dur, K, g, s)
        assert got["d_obs"].shape == got["d_rep"].shape == (n,) and got["d_obs"].dtype == got["d_rep"].dtype == np.float64
        assert np.isfinite(got["d_obs"]).all() and np.isfinite(got["d_rep"]).all()
        err = max(np.max(np.abs(got[k] - w) / np.maximum(np.abs(w), 1e-300)) for k, w in (("d_obs", d_obs), ("d_rep", d_rep)))
        WORST["err"] = max(WORST["err"], float(err))
        print(f"{g:8s}{s:14s} max rel err {err:.3e} (largest so far {WORST['err']:.3e})  p {got['p_value']:.4f}")
        np.testing.assert_allclose(got["d_obs"], d_obs, rtol=RTOL, atol=0, err_msg=f"d_obs {g} {s}")
        np.testing.assert_allclose(got["d_rep"], d_rep, rtol=RTOL, atol=0, err_msg=f"d_rep {g} {s}")
        # the p-value: exactly that of the returned arrays; the host function's up to the near ties, which are rare
        assert got["p_value"] == float(np.mean(got["d_rep"] > got["d_obs"]))
        gap = np.abs(got["d_rep"] - got["d_obs"])
        near = int(np.sum((gap > 0) & (gap <= 1e-9 * np.maximum(got["d_rep"], got["d_obs"]))))
        assert near <= n / 100, f"{near} near ties among {n} draws"
        extra = {k: opts[k] for k in ("session_duration", "max_abundance") if k in opts}
        p_host = posterior_predictive_check_counts(model, preds, data["obs"], g, s, **extra, **rates)
        assert abs(got["p_value"] - p_host) <= near / n + 1e-15, (got["p_value"], p_host, near)
        out[g, s] = got
    return out


# ------------------------------------------------------------------------------------------ equality with the definition ----
@pytest.mark.parametrize("name", MODELS)
def test_equals_the_definition(name):
    # one full 256-site block and a 44-site tail, two periods; occu_cop's durations reach 40: both branches of the Poisson sampler
    _compare(name, *_case(name, 0, N=300, T=2, J=3, n=64))


HANDLES = [("occu_rn", dict(fp="constant")), ("occu_cop", dict(fp="constant")), ("occu_cop", dict(fp="unoccupied")),
           ("nmixture", dict(re=True)), ("occu_rn", dict(re=True)), ("occu_cop", dict(re=True))]


@pytest.mark.parametrize("name,options", HANDLES, ids=[f"{m}-{'-'.join(map(str, o.values()))}-{'-'.join(o)}" for m, o in HANDLES])
def test_the_other_served_handles(name, options):
    data, posterior, opts = _case(name, 1, N=70, T=1, J=4, n=32, **options)
    got = _compare(name, data, posterior, opts)
    if name == "occu_cop":   # the host function takes the durations with or without the species axis
        preds, rates = predict(models.occu_cop, posterior, **data, num_samples=32, random_seed=5, **opts), _rates(name, posterior.sites)
        dur = opts["session_duration"]
        for g, s in PAIRS:
            a = posterior_predictive_check_counts(models.occu_cop, preds, data["obs"], g, s, session_duration=dur, **rates)
            b = posterior_predictive_check_counts(models.occu_cop, preds, data["obs"], g, s, session_duration=dur[None], **rates)
            assert a == b and abs(a - got[g, s]["p_value"]) <= 1 / 32


def test_a_truncation_that_bites():
    # max_abundance = 5 under an intercept of 3 (lambda ~ 20): the restricted mean is far below lambda, most N_i sit at the cap
    _compare("nmixture", *_case("nmixture", 8, N=70, T=2, J=3, n=32, max_abundance=5, intercept=3.0))


@pytest.mark.parametrize("name", ["nmixture", "occu_rn"])
def test_a_draw_whose_rate_passes_745(name):
    # draw 0 with an intercept of 10.5: lambda ~ 36000 exp(x . beta) > 745, where exp(-lambda) is 0 and lambda^n / n! overflows
    got = _compare(name, *_case(name, 9, N=70, T=1, J=3, n=16, hot_draw=10.5))
    assert all(np.isfinite(r["d_obs"][0]) and np.isfinite(r["d_rep"][0]) for r in got.values())


# ------------------------------------------------------------------------------------------ geometry ----
@pytest.mark.parametrize("N", [1, 257])
@pytest.mark.parametrize("name", MODELS)
def test_one_site_and_one_site_past_a_block(name, N):
    _compare(name, *_case(name, 3, N=N, T=2, J=2, n=16))


@pytest.mark.parametrize("name", MODELS)
def test_more_draws_than_grid_rows(name):
    data, posterior, opts = _case(name, 4, N=40, T=1, J=3, n=1100)   # the draw loop strides past grid_y = 1024
    _compare(name, data, posterior, opts, pairs=[("site", "chi-squared"), ("revisit", "freeman-tukey")])


def _handle(name, data, opts):
    extra = dict(session_duration=opts["session_duration"], fp_mode=None) if name == "occu_cop" else {}
    return OccuDataset(data["site_covs"], data["obs_covs"], np.full(data["obs"].shape, np.nan, dtype=np.float32), model=name, **extra)


@pytest.mark.parametrize("name", MODELS)
def test_same_bytes_twice_and_one_output_alone(name):
    data, posterior, opts = _case(name, 5, N=300, T=2, J=3, n=40)
    ds = _handle(name, data, opts)
    th = np.concatenate([posterior.sites["beta"][:, 0], posterior.sites["alpha"][:, 0]], axis=1)
    obs = data["obs"][0]
    a, b, c = (ds.predictive_check_counts(th, obs, seed=s) for s in (7, 7, 8))
    assert [x.shape for x in a] == [(40, 4), (40, 4)] and [x.dtype for x in a] == [np.float64, np.float64]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    # another seed: another replicate, the same observed side
    for k in (0, 1):
        assert np.array_equal(a[k][:, [0, 2]], c[k][:, [0, 2]]) and not np.array_equal(a[k][:, [1, 3]], c[k][:, [1, 3]])
    site_only, revisit_only = ds.predictive_check_counts(th, obs, seed=7, by_revisit=False), ds.predictive_check_counts(th, obs, seed=7, by_site=False)
    assert site_only[1] is None and revisit_only[0] is None
    assert site_only[0].tobytes() == a[0].tobytes() and revisit_only[1].tobytes() == a[1].tobytes()
    # a function of (seed, draw, period, site): the first draws of a longer call are the shorter call
    head = ds.predictive_check_counts(th[:7], obs, seed=7)
    assert head[0].tobytes() == a[0][:7].tobytes() and head[1].tobytes() == a[1][:7].tobytes()
    with pytest.raises(ValueError, match="counts or NaN"):
        ds.predictive_check_counts(th, np.where(np.isnan(obs), np.nan, -2.0), seed=7)
    with pytest.raises(ValueError, match="shape"):
        ds.predictive_check_counts(th, obs[:, :, :2], seed=7)
    ds.close()


# ------------------------------------------------------------------------------------------ masks ----
@pytest.mark.parametrize("name", MODELS)
def test_a_revisit_and_a_site_never_seen(name):
    data, posterior, opts = _case(name, 6, N=70, T=2, J=3, n=32)
    data["obs"][:, :, 1, 1] = np.nan   # one revisit never seen, with a later visit behind it: its draw is still taken
    data["obs"][:, 11] = np.nan        # one site never seen
    _compare(name, data, posterior, opts)
    # nothing seen at all: both sides are exactly 0, whatever the grouping
    ds = _handle(name, data, opts)
    th = np.concatenate([posterior.sites["beta"][:, 0], posterior.sites["alpha"][:, 0]], axis=1)
    by_site, by_revisit = ds.predictive_check_counts(th, np.full((70, 2, 3), np.nan), seed=1)
    assert not by_site.any() and not by_revisit.any()
    ds.close()


@pytest.mark.parametrize("name", MODELS)
def test_missing_covariates_read_as_zero(name):
    data, posterior, opts = _case(name, 7, N=70, T=2, J=3, n=32)
    data["site_covs"][4, 1] = data["obs_covs"][7, 1, 2, 0] = data["obs_covs"][69, 0, 0, 1] = np.nan
    with_holes = _compare(name, data, posterior, opts)
    filled = {**data, "site_covs": np.nan_to_num(data["site_covs"]), "obs_covs": np.nan_to_num(data["obs_covs"])}
    for (g, s), want in with_holes.items():
        got = predictive_check_counts(getattr(models, name), posterior, **filled, group_by=g, statistic=s, random_seed=5, **opts)
        assert got["d_obs"].tobytes() == want["d_obs"].tobytes() and got["d_rep"].tobytes() == want["d_rep"].tobytes()


# ------------------------------------------------------------------------------------------ a real fit ----
def test_a_small_fit():
    with contextlib.redirect_stdout(io.StringIO()):
        data, _ = simulate_nmixture(n_sites=60, deployment_days_per_site=35, random_seed=1)
    K = int(np.nanmax(data["obs"])) + 5
    res = fit(models.nmixture, **data, max_abundance=K, num_chains=1, num_samples=100, num_warmup=100, timeout=600)
    preds = predict(models.nmixture, res.mcmc, **data, max_abundance=K, num_samples=100, random_seed=3)
    for g, s in PAIRS:
        got = predictive_check_counts(models.nmixture, res.mcmc, **data, max_abundance=K, group_by=g, statistic=s, random_seed=3)
        assert 0.0 <= got["p_value"] <= 1.0
        assert got["p_value"] == posterior_predictive_check_counts(models.nmixture, preds, data["obs"], g, s, max_abundance=K)


# ------------------------------------------------------------------------------------------ the C-ABI's refusals ----
def test_refusals_at_the_abi():
    with contextlib.redirect_stdout(io.StringIO()):
        data, _ = simulate(n_sites=20, random_seed=0)
    n = 2

    def call(ds, obs, *outs):
        dr = np.zeros((n, ds.D), dtype=np.float32)
        ptrs = [None if o is None else o.ctypes.data_as(C.POINTER(C.c_double)) for o in outs]
        return ds._lib.bl_predictive_check_counts(ds._h, n, dr.ctypes.data_as(C.POINTER(C.c_float)), 0,
                                                  None if obs is None else obs.ctypes.data_as(C.POINTER(C.c_int32)), *ptrs)

    # handles the entry does not serve: the message names the model, and an occu handle is pointed to its own entry
    for name, ds in {"occu": OccuDataset(data["site_covs"], data["obs_covs"], data["obs"]),
                     "occu_cs": OccuDataset(data["site_covs"], data["obs_covs"], data["obs"], model="occu_cs")}.items():
        obs, out = np.zeros(ds.J * ds.T * ds.N, dtype=np.int32), np.zeros((2, n, 4))
        assert call(ds, obs, out[0], out[1]) == _ffi.BL_ERR_UNSUPPORTED
        msg = ds._lib.bl_last_error()
        assert b"bl_predictive_check_counts: not built for " + name.encode() in msg and b"occu uses bl_predictive_check)" in msg
        assert call(ds, obs, None, None) == _ffi.BL_ERR_INVALID
        assert not out.any()
        with pytest.raises(NotImplementedError, match=name):
            ds.predictive_check_counts(np.zeros((n, ds.D), dtype=np.float32), np.zeros((ds.N, ds.T, ds.J)))
        ds.close()
    # a served handle: every output NULL, no observations, an observation below -1, and one above 1 on occu_rn
    ds = OccuDataset(data["site_covs"], data["obs_covs"], data["obs"], model="occu_rn", max_abundance=20)
    obs, out = np.zeros(ds.J * ds.T * ds.N, dtype=np.int32), np.zeros((n, 4))
    assert call(ds, obs, None, None) == _ffi.BL_ERR_INVALID
    assert call(ds, None, out, None) == _ffi.BL_ERR_INVALID
    obs[3] = -2
    assert call(ds, obs, out, None) == _ffi.BL_ERR_INVALID and b"obs holds -2" in ds._lib.bl_last_error()
    obs[3] = 2
    assert call(ds, obs, None, out) == _ffi.BL_ERR_INVALID and b"obs holds 2" in ds._lib.bl_last_error()
    assert not out.any()
    obs[3] = -1
    assert call(ds, obs, out, None) == _ffi.BL_OK and out.any()
    ds.close()
    # ... which a count handle takes
    ds = OccuDataset(data["site_covs"], data["obs_covs"], data["obs"], model="nmixture", max_abundance=20)
    obs[3] = 2
    assert call(ds, obs, out, None) == _ffi.BL_OK
    ds.close()
