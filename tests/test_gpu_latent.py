"""bl_site_posterior on the device against the float64 restatement in tests/latent_ref.py: per-cell parity at random theta for every
served family, the exact structure (empty cells, detections without false positives), the sum identity with the sampler's own density
on the same handle, the draws, the chunk boundary, the refusals, and fit -> conditional_occupancy end to end.

Bounds (tests/latent_ref.py: bounds): |l32 - l64| <= rtol S + ulp32(l64) / 2 with S the sum of the absolute values of the cell's terms
and rtol the family's committed bl_logp_grad bound (1e-6 occu and false positives: test_gpu_logp.py, test_gpu_fp.py; 2e-6 random
effects and occu_comb: test_gpu_re.py, test_gpu_re_fp.py, test_gpu_comb.py); |q32 - q64| <= (bound on A + bound on B) / 4 + 2^-23.
Every check prints the largest measured error as a fraction of its bound (pytest -s).  Measured on an MI355X, largest over the cases
of each family, as (log_lik, z_prob, sum identity) / bound: plain occu 0.082, 0.132, 0.143 (bound rtol 1e-6); false positives 0.091,
0.122, 0.115 (1e-6); random effects, with and without a rate 0.042, 0.073, 0.053 (2e-6); occu_comb 0.043, 0.096, 0.035 (2e-6); the
chunk-boundary sample 0.141.  Draws: 1 834 593 cells in range, standardised sum 1.53 (bound 4.5)."""
import contextlib
import ctypes as C
import io
import math
import time

import numpy as np
import pytest
from scipy import stats

import latent_ref as L
from biolith_amd import _ffi
from biolith_amd.engine import OccuDataset
from biolith_amd.evaluation import finite_sample_occupancy, residuals, waic_marginal
from biolith_amd.models import occu, occu_comb, simulate, simulate_comb
from biolith_amd.utils import conditional_occupancy, fit, predict
from comb_ref import REF_INDEX, CombRef, from_data, reference_case
from conftest import quiet_simulate

pytestmark = pytest.mark.gpu


def _check(ds, cells_of, th, rtol, log_prior=None, no_fp=False, tag=""):
    """Parity, structure and sum identity of one handle at the thetas th (B, D)."""
    th = np.asarray(th, dtype=np.float32).astype(np.float64)
    ll, q, z = ds.site_posterior(th, seed=5)
    assert ll.shape == q.shape == z.shape == (th.shape[0], ds.T, ds.N) and ll.dtype == q.dtype == np.float32 and z.dtype == np.uint8
    assert np.all(np.isfinite(ll)) and np.all((q >= 0) & (q <= 1)) and set(np.unique(z)) <= {0, 1}
    worst_l = worst_q = worst_s = 0.0
    U = ds.logp_grad(th)[0] if log_prior is not None else None
    for b in range(th.shape[0]):
        c = cells_of(th[b])
        bl, bq = L.bounds(c, rtol)
        el, eq = np.abs(ll[b] - c["l"]), np.abs(q[b] - c["q"])
        worst_l, worst_q = max(worst_l, float(np.max(el / bl))), max(worst_q, float(np.max(eq / bq)))
        assert np.all(el <= bl), (tag, b, float(np.max(el / bl)))
        assert np.all(eq <= bq), (tag, b, float(np.max(eq / bq)))
        empty = c["n_obs"] == 0
        assert np.all(ll[b][empty] == 0.0)           # exactly: nothing observed, likelihood 1
        if no_fp:   # a detection proves occupancy
            det = c["B"] < -80.0   # B carries at least one log(tiny) = -87.3 (log(1 - psi) is O(1) at these thetas)
            assert det.any()
            assert np.all(q[b][det] >= 1 - 2.0 ** -24) and np.all(z[b][det] == 1)
        if U is not None:   # the new kernel's cells add up to the likelihood part of the sampler's own potential
            want = -U[b] - log_prior(th[b])
            worst_s = max(worst_s, abs(float(ll[b].astype(np.float64).sum()) - want) / (rtol * abs(want)))
            assert abs(float(ll[b].astype(np.float64).sum()) - want) <= rtol * abs(want), (tag, b, ll[b].sum(), want)
    print(f"\n[{tag}] max error / bound: log_lik {worst_l:.3f}, z_prob {worst_q:.3f}, sum identity {worst_s:.3f}")
    return ll, q, z


def _normal_lp(x, loc=0.0, scale=1.0):
    return float(np.sum(stats.norm.logpdf(x, loc, scale)))


def _beta_logit_lp(phi, a=2.0, b=5.0):
    f = 1.0 / (1.0 + math.exp(-phi))
    return float(stats.beta.logpdf(f, a, b) + math.log(f) + math.log1p(-f))


def _occu_arrays(T, Ks, Ko, N=300, J=4, seed=0):
    rng = np.random.default_rng(seed)
    X, W = rng.normal(size=(N, Ks)), rng.normal(size=(N, T, J, Ko))
    Y = (rng.uniform(size=(1, N, T, J)) < 0.3).astype(np.float64)
    Y[rng.uniform(size=Y.shape) < 0.3] = np.nan
    Y[0, :4] = np.nan
    if Ks:
        X[6, 0] = np.nan
    if Ko:
        W[8, 0, 1, 0] = np.nan
    return X, W, Y


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("ks,ko", [(0, 0), (3, 3), (16, 16)])
def test_plain_occu_parity(ks, ko, T):
    if ks == 3:   # the simulator's own missingness (simulate_missing=True)
        data, _, _ = quiet_simulate(n_sites=200, n_site_covs=ks, n_obs_covs=ko, n_periods=T, deployment_days_per_site=42, simulate_missing=True, random_seed=T)
        X, W, Y = data["site_covs"], data["obs_covs"], data["obs"]
    else:
        X, W, Y = _occu_arrays(T, ks, ko, seed=ks + T)
    ds = OccuDataset(X, W, Y)
    rng = np.random.default_rng(10 * ks + T)
    th = rng.uniform(-2, 2, size=(4, ds.D)) * (1.0 if ks <= 3 else 0.35)
    lp = lambda t: _normal_lp(t)
    _check(ds, lambda t: L.occu_cells(X, W, Y[0], t), th, 1e-6, log_prior=lp, no_fp=True, tag=f"occu T={T} K=({ks},{ko})")
    ds.close()


@pytest.mark.parametrize("mode", ["constant", "unoccupied"])
def test_false_positive_parity(mode):
    X, W, Y = _occu_arrays(2, 2, 2, seed=3)
    ds = OccuDataset(X, W, Y, model="occu_fp", fp_mode=mode)
    th = np.random.default_rng(2).uniform(-2, 2, size=(4, ds.D))
    th[0, -1], th[1, -1] = -6.0, 4.0
    lp = lambda t: _normal_lp(t[:-1]) + _beta_logit_lp(t[-1])
    _check(ds, lambda t: L.occu_cells(X, W, Y[0], t, fp_mode=mode), th, 1e-6, log_prior=lp, tag=f"occu_fp {mode}")
    ds.close()


def _re_log_prior(t, N, T, J, Ks, Ko, fp, site, obs, scales=(1.0, 1.0)):
    o = L.occu_theta_layout(N, T, J, Ks, Ko, fp, site, obs)
    lp, at = _normal_lp(t[:Ks + Ko + 2]), Ks + Ko + 2
    if fp:
        lp += _beta_logit_lp(t[at])
        at += 1
    sds = []
    for on, sc in ((site, scales[0]), (obs, scales[1])):   # sd ~ HalfNormal(scale) in log sd: + log sd
        if on:
            lp += float(stats.halfnorm.logpdf(math.exp(t[at]), scale=sc)) + t[at]
            sds.append(math.exp(t[at]))
            at += 1
    if site:
        lp += _normal_lp(t[o["u"]:o["u"] + 2 * N], 0.0, sds[0])
    if obs:
        lp += _normal_lp(t[o["e"]:o["e"] + N * T * J], 0.0, sds[-1])
    return lp


@pytest.mark.parametrize("site,obs,fp", [(True, False, None), (False, True, None), (True, True, None), (True, True, "constant"), (True, False, "unoccupied")])
def test_random_effects_parity(site, obs, fp):
    X, W, Y = _occu_arrays(2, 2, 3, N=150, seed=7)
    ds = OccuDataset(X, W, Y, model="occu_re", site_random_effects=site, obs_random_effects=obs, re_fp_mode=fp)
    th = np.random.default_rng(4).uniform(-1.2, 1.2, size=(3, ds.D))
    lp = lambda t: _re_log_prior(t, 150, 2, 4, 2, 3, fp is not None, site, obs)
    _check(ds, lambda t: L.occu_cells(X, W, Y[0], t, fp_mode=fp, site_re=site, obs_re=obs), th, 2e-6, log_prior=lp, no_fp=fp is None,
           tag=f"occu_re site={site} obs={obs} fp={fp}")
    ds.close()


def _comb_ds(data, **pri):
    kw = {}
    if pri:
        from biolith_amd.distributions import LocScale
        kw = dict(prior_beta=LocScale(*pri["prior_beta"][:2], family=pri["prior_beta"][2]), prior_alpha=LocScale(*pri["prior_alpha"][:2], family=pri["prior_alpha"][2]),
                  prior_fc=pri["prior_fc"], prior_fu=pri["prior_fu"], prior_mu=pri["prior_mu"], prior_sigma=pri["prior_sigma"])
    return OccuDataset(data["site_covs"], data["PC_obs_covs"], data["PC_obs"][:1], model="occu_comb", ARU_obs_covs=data["ARU_obs_covs"],
                       ARU_obs=data["ARU_obs"][:1], scores_obs=data["scores_obs"][:1], **kw)


def _comb_theta(rng, ref, n):   # (test_gpu_comb.py: _theta)
    o = ref.D - 6
    th = rng.uniform(-1, 1, size=(n, ref.D)) * np.r_[np.full(o, 0.7), np.ones(6)]
    th[:, o:] = np.array([-1.2, -1.5, -2.0, math.log(5.0), math.log(4.5), math.log(3.0)]) + rng.uniform(-0.4, 0.4, size=(n, 6))
    return th


@pytest.mark.parametrize("case", sorted(REF_INDEX))
def test_comb_parity_reference_cases(case):
    data, pri, fx = reference_case(case)
    ref = CombRef(data["site_covs"], data["PC_obs_covs"], data["ARU_obs_covs"], data["PC_obs"][:1], data["ARU_obs"][:1], data["scores_obs"][:1], **pri)
    ds = _comb_ds(data, **pri)
    th = np.vstack([np.asarray([p["theta"] for p in fx["points"]]), _comb_theta(np.random.default_rng(1), ref, 2)])
    _check(ds, lambda t: L.comb_cells(ref, t), th, 2e-6, log_prior=ref.log_prior, tag=f"comb {case}")
    ds.close()


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("ks,kpc,karu", [(1, 1, 1), (3, 0, 2), (4, 4, 4), (6, 9, 16), (16, 16, 16)])
def test_comb_parity_shapes(ks, kpc, karu, T):
    with contextlib.redirect_stdout(io.StringIO()):
        data, _ = simulate_comb(n_site_covs=ks, n_PC_covs=kpc, n_ARU_covs=karu, n_sites=40, n_periods=T, PC_replicates=3, ARU_replicates=7,
                                scores_replicates=5, ARU_prob_fp_constant=0.05, ARU_prob_fp_unoccupied=0.1, simulate_missing=True, random_seed=ks + 7 * T)
    ref, ds = from_data(data), _comb_ds(data)
    th = _comb_theta(np.random.default_rng(ks * 100 + kpc * 10 + karu + T), ref, 2)
    _check(ds, lambda t: L.comb_cells(ref, t), th, 2e-6, log_prior=ref.log_prior, tag=f"comb K=({ks},{kpc},{karu}) T={T}")
    ds.close()


def test_comb_parity_many_sites():
    with contextlib.redirect_stdout(io.StringIO()):
        data, _ = simulate_comb(n_sites=5000, n_periods=2, ARU_prob_fp_constant=0.05, ARU_prob_fp_unoccupied=0.1, simulate_missing=True, random_seed=2)
    ref, ds = from_data(data), _comb_ds(data)
    _check(ds, lambda t: L.comb_cells(ref, t), _comb_theta(np.random.default_rng(0), ref, 2), 2e-6, log_prior=ref.log_prior, tag="comb 5000 sites")
    ds.close()


def test_draws_are_seeded_and_calibrated():
    N, T, J, n = 4000, 2, 3, 400
    rng = np.random.default_rng(11)
    X, W = rng.normal(size=(N, 2)), rng.normal(size=(N, T, J, 1))
    Y = (rng.uniform(size=(1, N, T, J)) < 0.15).astype(np.float64)
    th = (np.array([0.0, 0.5, -0.5, -0.6, 0.4]) + rng.normal(scale=0.3, size=(n, 5))).astype(np.float32)
    # the restatement's own q leaves enough cells in range (float64, no device)
    q64 = np.stack([L.occu_cells(X, W, Y[0], t)["q"] for t in th.astype(np.float64)])
    assert ((q64 > 0.05) & (q64 < 0.95)).sum() >= 10 ** 6
    ds = OccuDataset(X, W, Y)
    _, q, z = ds.site_posterior(th, seed=1)
    _, _, z_same = ds.site_posterior(th, seed=1, log_lik=False, z_prob=False)
    _, _, z_other = ds.site_posterior(th, seed=2, log_lik=False, z_prob=False)
    assert z.tobytes() == z_same.tobytes() and z.tobytes() != z_other.tobytes()
    _, _, z_part = ds.site_posterior(th[:7], seed=1, log_lik=False, z_prob=False)   # (seed, draw, period, site) only
    assert np.array_equal(z_part, z[:7])
    m = (q > 0.05) & (q < 0.95)
    assert m.sum() >= 10 ** 6
    qd = q[m].astype(np.float64)
    stat = float((z[m].astype(np.float64) - qd).sum() / math.sqrt((qd * (1 - qd)).sum()))
    print(f"\n[draws] {m.sum()} cells in range, standardised sum of z - z_prob = {stat:.3f}")
    assert abs(stat) <= 4.5
    ds.close()


def test_chunk_boundary():
    N, n = 20000, 4000   # log_lik: 320 MB, more than one 256 MB chunk of device scratch
    rng = np.random.default_rng(3)
    X, W = rng.normal(size=(N, 1)), rng.normal(size=(N, 1, 3, 1))
    Y = (rng.uniform(size=(1, N, 1, 3)) < 0.2).astype(np.float64)
    Y[rng.uniform(size=Y.shape) < 0.2] = np.nan
    th = rng.uniform(-1.5, 1.5, size=(n, 4)).astype(np.float32)
    ds = OccuDataset(X, W, Y)
    ll, q, z = ds.site_posterior(th, seed=9)
    assert ll.nbytes > (256 << 20)
    worst = 0.0
    for b in (0, 1, 3354, 3355, n - 2, n - 1):   # both sides of the boundary (3355 draws of 80 kB fill a chunk), first and last draw
        c = L.occu_cells(X, W, Y[0], th[b].astype(np.float64))
        bl, bq = L.bounds(c, 1e-6)
        cells = np.random.default_rng(b).choice(N, size=2000, replace=False)
        el, eq = np.abs(ll[b][:, cells] - c["l"][:, cells]), np.abs(q[b][:, cells] - c["q"][:, cells])
        worst = max(worst, float(np.max(el / bl[:, cells])), float(np.max(eq / bq[:, cells])))
        assert np.all(el <= bl[:, cells]) and np.all(eq <= bq[:, cells]), b
    _, _, z_tail = ds.site_posterior(th[:3], seed=9, log_lik=False, z_prob=False)
    assert np.array_equal(z_tail, z[:3])
    print(f"\n[chunks] max error / bound on the sampled cells: {worst:.3f}")
    ds.close()


def test_abi_refusals_and_busy():
    data, _, _ = quiet_simulate(n_sites=60, deployment_days_per_site=28, random_seed=1)
    X, W, Y = data["site_covs"], data["obs_covs"], data["obs"]
    cnt = np.nan_to_num(Y) * 2
    handles = [("occu_rn", OccuDataset(X, W, Y, model="occu_rn", max_abundance=20)), ("nmixture", OccuDataset(X, W, cnt, model="nmixture", max_abundance=20)),
               ("occu_cop", OccuDataset(X, W, cnt, model="occu_cop", fp_mode=None, session_duration=np.ones(Y.shape[1:]))),
               ("occu_cs", OccuDataset(X, W, np.where(np.isnan(Y), np.nan, Y * 2.0 - 1.0), model="occu_cs")), ("occu_dyn", OccuDataset(X, W, Y, model="occu_dyn")),
               ("joint-species", OccuDataset(X, W, np.concatenate([Y, Y])))]
    for name, ds in handles:
        dr = np.zeros((2, ds.D), dtype=np.float32)
        out = np.zeros((2, ds.T, ds.N), dtype=np.float32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        assert ds._lib.bl_site_posterior(ds._h, 2, fp(dr), 0, fp(out), None, None) == _ffi.BL_ERR_UNSUPPORTED, name
        assert name in ds._lib.bl_last_error().decode(), (name, ds._lib.bl_last_error())
        with pytest.raises(NotImplementedError):
            ds.site_posterior(dr)
        ds.close()
    ds = OccuDataset(X, W, Y)
    assert ds._lib.bl_site_posterior(ds._h, 0, None, 0, None, None, None) == _ffi.BL_ERR_INVALID
    big, _, _ = quiet_simulate(n_sites=4000, n_site_covs=2, n_obs_covs=2, deployment_days_per_site=140)
    db = OccuDataset(big["site_covs"], big["obs_covs"], big["obs"])
    db.launch(num_warmup=200000, num_samples=200000, num_chains=2, seed=0)
    time.sleep(0.2)
    assert not db.done()
    with pytest.raises(_ffi.EngineError) as ei:
        db.site_posterior(np.zeros((1, db.D), dtype=np.float32))
    assert ei.value.code == _ffi.BL_ERR_BUSY
    db.abort()
    with pytest.raises(Exception, match="aborted"):
        db.wait()
    assert db.site_posterior(np.zeros((1, db.D), dtype=np.float32))[0].shape == (1, db.T, db.N)   # the handle stays usable
    db.close()
    ds.close()


def _brier(p, truth):
    return float(np.mean((p - truth) ** 2))


def test_end_to_end_occu():
    data, truth, _ = quiet_simulate(n_sites=400, n_site_covs=2, n_obs_covs=2, deployment_days_per_site=35, simulate_missing=True, random_seed=3)
    res = fit(occu, **data, num_chains=2, num_warmup=300, num_samples=250)
    lat = conditional_occupancy(occu, res.mcmc, **data, random_seed=4)
    n, T, N = 500, 1, 400
    assert list(lat) == ["psi", "z_prob", "z", "log_lik", "n_obs"]
    for k, dt in (("psi", np.float32), ("z_prob", np.float32), ("z", np.int32), ("log_lik", np.float32)):
        assert lat[k].shape == (n, T, N, 1) and lat[k].dtype == dt, k
    assert lat["n_obs"].shape == (T, N, 1) and lat["n_obs"].dtype == np.int32
    np.testing.assert_allclose(lat["psi"], res.samples["psi"], rtol=0, atol=0)
    zt = np.asarray(truth["z"], dtype=np.float64).reshape(N)
    b_q, b_psi = _brier(lat["z_prob"].mean(0)[0, :, 0], zt), _brier(lat["psi"].mean(0)[0, :, 0], zt)
    print(f"\n[occu e2e] Brier: z_prob {b_q:.4f}, psi {b_psi:.4f}")
    assert b_q < b_psi
    assert abs(float(finite_sample_occupancy(lat).mean()) - truth["z"].mean()) < 0.1
    w = waic_marginal(lat)
    assert all(np.isfinite(v) for v in w.values()) and w["p_waic"] > 0
    preds = predict(occu, res.mcmc, **data, num_samples=n)
    o, d = residuals({**preds, "z": lat["z"]}, data["obs"])
    assert o.shape == (n, T, N, 1) and np.all(np.abs(o) <= 1)
    X, W, Y = (np.asarray(data[k], dtype=np.float64) for k in ("site_covs", "obs_covs", "obs"))
    seen = ~(np.isnan(Y[0]) | np.isnan(W).any(-1) | np.isnan(X).any(-1)[:, None, None])   # a masked visit's y does not count
    det = ((np.nan_to_num(Y[0]) > 0) & seen).any(axis=(1, 2))
    assert det.sum() > 50
    assert np.all(lat["z"][:, 0, det, 0] == 1)   # a site with a detection is occupied in every conditional draw


def test_end_to_end_comb():
    with contextlib.redirect_stdout(io.StringIO()):
        data, truth = simulate_comb(n_sites=300, ARU_prob_fp_constant=0.05, ARU_prob_fp_unoccupied=0.1, simulate_missing=True, random_seed=1)
    res = fit(occu_comb, **data, num_chains=2, num_warmup=300, num_samples=250)
    lat = conditional_occupancy(occu_comb, res.mcmc, **data)
    n, T, N = 500, 1, 300
    for k in ("psi", "z_prob", "z", "log_lik"):
        assert lat[k].shape == (n, T, N, 1), k
    assert lat["n_obs"].shape == (T, N, 1) and lat["z"].dtype == np.int32
    np.testing.assert_allclose(lat["psi"], res.samples["psi"], rtol=2e-6, atol=1e-7)
    zt = np.asarray(truth["z"], dtype=np.float64)[0, 0]     # (S, T, N)
    b_q, b_psi = _brier(lat["z_prob"].mean(0)[0, :, 0], zt), _brier(lat["psi"].mean(0)[0, :, 0], zt)
    print(f"\n[comb e2e] Brier: z_prob {b_q:.4f}, psi {b_psi:.4f}")
    assert b_q < b_psi
    assert abs(float(finite_sample_occupancy(lat).mean()) - truth["z"].mean()) < 0.1
    w = waic_marginal(lat)
    assert all(np.isfinite(v) for v in w.values()) and w["p_waic"] > 0
