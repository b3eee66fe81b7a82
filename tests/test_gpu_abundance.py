"""bl_abundance_posterior on the device against the float64 restatement in tests/abundance_ref.py: per-cell parity for every served handle
kind, the sum identity with the sampler's own density on the same handle, the draws, the chunk boundary, the ABI's refusals, and
fit -> conditional_abundance end to end.

Bounds (tests/abundance_ref.py: bounds): |l32 - l64| <= rtol S + ulp32(l64) / 2 with S the pmf-weighted mean over n of the sum of the
absolute values of the terms of l_n and rtol the family's committed bl_logp_grad bound (occu_rn 1e-5; nmixture and
the random-effects handles 2e-6); N_mean: that bound times the pmf's sd plus an ulp; occ_prob: half of it plus 2^-23.  Every check prints
the largest measured error as a fraction of its bound (pytest -s); the figures measured on an MI355X are in DESIGN.md section 5."""
import contextlib
import ctypes as C
import io
import math
import time

import numpy as np
import pytest
from scipy import stats

import abundance_ref as A
from biolith_amd import _ffi
from biolith_amd.engine import OccuDataset
from biolith_amd.evaluation import finite_sample_abundance, lppd_marginal, waic_marginal
from biolith_amd.models import nmixture, occu, occu_rn, simulate_comb, simulate_nmixture, simulate_rn
from biolith_amd.utils import conditional_abundance, conditional_occupancy, fit, predict
from conftest import quiet_simulate

pytestmark = pytest.mark.gpu


def _sim(fn, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(**kw)


def _check(ds, cells_of, th, rtol, log_prior=None, tag=""):
    """Parity, structure and sum identity of one handle at the thetas th (B, D)."""
    th = np.asarray(th, dtype=np.float32).astype(np.float64)
    ll, mean, occ, draw = ds.abundance_posterior(th, seed=5)
    shape = (th.shape[0], ds.T, ds.N)
    assert ll.shape == mean.shape == occ.shape == draw.shape == shape
    assert ll.dtype == mean.dtype == occ.dtype == np.float32 and draw.dtype == np.int32
    assert np.all(np.isfinite(ll)) and np.all((occ >= 0) & (occ <= 1)) and np.all((draw >= 0) & (draw <= ds.max_abundance))
    worst = np.zeros(4)
    U = ds.logp_grad(th)[0] if log_prior is not None else None
    for b in range(th.shape[0]):
        c = cells_of(th[b])
        bl, bm, bo = A.bounds(c, rtol)
        el, em, eo = np.abs(ll[b] - c["l"]), np.abs(mean[b] - c["mean"]), np.abs(occ[b] - c["occ"])
        worst[:3] = np.maximum(worst[:3], [np.max(el / bl), np.max(em / bm), np.max(eo / bo)])
        print(f"[{tag}] theta {b}: error / bound log_lik {np.max(el / bl):.3f}, N_mean {np.max(em / bm):.3f}, occ_prob {np.max(eo / bo):.3f}")
        assert np.all(el <= bl), (tag, b, float(np.max(el / bl)))
        assert np.all(em <= bm), (tag, b, float(np.max(em / bm)))
        assert np.all(eo <= bo), (tag, b, float(np.max(eo / bo)))
        assert np.all(c["pmf"][np.arange(ds.T)[:, None], np.arange(ds.N)[None, :], draw[b]] > 0)   # a draw has mass
        if U is not None:   # the new kernel's cells add up to the likelihood part of the sampler's own potential
            want = -U[b] - log_prior(th[b])
            got = float(ll[b].astype(np.float64).sum())
            worst[3] = max(worst[3], abs(got - want) / (rtol * abs(want)))
            print(f"[{tag}] theta {b}: sum identity error / bound {abs(got - want) / (rtol * abs(want)):.3f}")
            assert abs(got - want) <= rtol * abs(want), (tag, b, got, want)
    print(f"[{tag}] max error / bound: log_lik {worst[0]:.3f}, N_mean {worst[1]:.3f}, occ_prob {worst[2]:.3f}, sum identity {worst[3]:.3f}")
    return ll, mean, occ, draw


def _thetas(rng, D, truth, Ks, Ko, wide):
    """Three init_to_uniform-like points (uniform on (-2, 2), narrower with many covariates so that lambda stays a count) and one
    near the simulator's truth; the coordinates behind the coefficients (rate, log sds, effects) at half the width."""
    th = rng.uniform(-2, 2, size=(4, D)) * (1.0 if not wide else 0.35)
    th[:, Ks + Ko + 2:] *= 0.5
    th[3, :Ks + Ko + 2] = np.r_[np.asarray(truth["beta"]).reshape(-1)[:Ks + 1], np.asarray(truth["alpha"]).reshape(-1)[:Ko + 1]] + rng.normal(scale=0.05, size=Ks + Ko + 2)
    return th


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("ks,ko", [(1, 1), (3, 3), (8, 16)])
def test_rn_parity(ks, ko, T):
    data, truth = _sim(simulate_rn, n_sites=150, n_site_covs=ks, n_obs_covs=ko, n_periods=T, deployment_days_per_site=42, simulate_missing=True, random_seed=ks + T)
    X, W, Y = data["site_covs"], data["obs_covs"], data["obs"]
    N, _, J, _ = W.shape
    for K in (20, 100):
        ds = OccuDataset(X, W, Y, model="occu_rn", max_abundance=K)
        th = _thetas(np.random.default_rng(10 * ks + T + K), ds.D, truth, ks, ko, ks > 3)
        _check(ds, lambda t: A.rn_cells(X, W, Y[0], t, K), th, 1e-5, log_prior=lambda t: A.log_prior(t, N, T, J, ks, ko), tag=f"occu_rn T={T} K=({ks},{ko}) max={K}")
        ds.close()


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("ks,ko", [(1, 1), (3, 3), (8, 16)])
def test_nmix_parity(ks, ko, T):
    data, truth = _sim(simulate_nmixture, n_sites=150, n_site_covs=ks, n_obs_covs=ko, n_periods=T, deployment_days_per_site=42, simulate_missing=True, random_seed=ks + T)
    X, W, Y = data["site_covs"], data["obs_covs"], data["obs"]
    N, _, J, _ = W.shape
    for K in (int(max(20, np.nanmax(Y))), 100):
        ds = OccuDataset(X, W, Y, model="nmixture", max_abundance=K)
        th = _thetas(np.random.default_rng(10 * ks + T + K), ds.D, truth, ks, ko, ks > 3)
        _check(ds, lambda t: A.nmix_cells(X, W, Y[0], t, K), th, 2e-6, log_prior=lambda t: A.log_prior(t, N, T, J, ks, ko), tag=f"nmixture T={T} K=({ks},{ko}) max={K}")
        ds.close()


@pytest.mark.parametrize("ks,ko", [(2, 3), (8, 16)])
@pytest.mark.parametrize("site,obs,fp", [(True, False, False), (False, True, False), (True, True, False), (False, False, True), (True, True, True)])
def test_rn_effects_and_rate_parity(site, obs, fp, ks, ko):
    """The random-effects framework's Royle-Nichols handles: kind 4 (effects) and kind 5 (a false-positive rate, with or without effects),
    at both capacities those kernels are built for (4 and 16 covariates per side: the rows' padding differs)."""
    T = 2
    data, truth = _sim(simulate_rn, n_sites=120, n_site_covs=ks, n_obs_covs=ko, n_periods=T, deployment_days_per_site=28, simulate_missing=True, random_seed=7)
    X, W, Y = data["site_covs"], data["obs_covs"], data["obs"]
    N, _, J, _ = W.shape
    for K in (20, 100):
        ds = OccuDataset(X, W, Y, model="occu_rn", max_abundance=K, site_random_effects=site, obs_random_effects=obs, re_fp_mode="constant" if fp else None)
        th = _thetas(np.random.default_rng(4 + K), ds.D, truth, ks, ko, ks > 3)
        if fp:
            th[0, ks + ko + 2], th[1, ks + ko + 2] = -6.0, 2.0
        _check(ds, lambda t: A.rn_cells(X, W, Y[0], t, K, fp=fp, site_re=site, obs_re=obs), th, 2e-6,
               log_prior=lambda t: A.log_prior(t, N, T, J, ks, ko, fp, site, obs), tag=f"occu_rn site={site} obs={obs} fp={fp} K=({ks},{ko}) max={K}")
        ds.close()


@pytest.mark.parametrize("ks,ko", [(2, 3), (8, 16)])
@pytest.mark.parametrize("site,obs", [(True, False), (False, True), (True, True)])
def test_nmix_effects_parity(site, obs, ks, ko):
    T = 2
    data, truth = _sim(simulate_nmixture, n_sites=120, n_site_covs=ks, n_obs_covs=ko, n_periods=T, deployment_days_per_site=28, simulate_missing=True, random_seed=7)
    X, W, Y = data["site_covs"], data["obs_covs"], data["obs"]
    N, _, J, _ = W.shape
    for K in (int(max(20, np.nanmax(Y))), 100):
        ds = OccuDataset(X, W, Y, model="nmixture", max_abundance=K, site_random_effects=site, obs_random_effects=obs)
        th = _thetas(np.random.default_rng(9 + K), ds.D, truth, ks, ko, ks > 3)
        _check(ds, lambda t: A.nmix_cells(X, W, Y[0], t, K, site_re=site, obs_re=obs), th, 2e-6,
               log_prior=lambda t: A.log_prior(t, N, T, J, ks, ko, False, site, obs), tag=f"nmixture site={site} obs={obs} K=({ks},{ko}) max={K}")
        ds.close()


@pytest.mark.parametrize("model", ["occu_rn", "nmixture"])
def test_draws_are_seeded_and_calibrated(model):
    """4 000 copies of one theta: 4 000 independent N_i per cell.  The standardised cell means are asserted where the central limit
    theorem carries them (a cell whose pmf has sd >= 0.2: 4 000 draws then hold at least 160 units of variance).  A cell below that sits
    on its mode with rare neighbours: its mean cannot be standardised (sd may be 0) and is far from normal, so each such cell is held to
    the exact law of what it shows instead -- the number of its draws off the mode is Binomial(4 000, 1 - pmf(mode)) and must lie between
    that law's 1e-7 and 1 - 1e-7 quantiles (at most 600 cells, two sides: a false alarm below 2e-4); a cell whose pmf is one value to
    rounding must return that value in every draw.  The pooled chi-square then takes every cell."""
    n, K = 4000, 40
    sim = simulate_rn if model == "occu_rn" else simulate_nmixture
    data, truth = _sim(sim, n_sites=300, n_periods=2, deployment_days_per_site=35, simulate_missing=True, random_seed=11)
    X, W, Y = data["site_covs"], data["obs_covs"], data["obs"]
    K = int(max(K, np.nanmax(Y)))
    th1 = np.r_[np.asarray(truth["beta"]).reshape(-1), np.asarray(truth["alpha"]).reshape(-1)].astype(np.float32)
    c = (A.rn_cells if model == "occu_rn" else A.nmix_cells)(X, W, Y[0], th1.astype(np.float64), K)
    ds = OccuDataset(X, W, Y, model=model, max_abundance=K)
    th = np.tile(th1, (n, 1))
    _, _, _, d = ds.abundance_posterior(th, seed=1)
    d_same = ds.abundance_posterior(th, seed=1, log_lik=False, n_mean=False, occ_prob=False)[3]
    d_other = ds.abundance_posterior(th, seed=2, log_lik=False, n_mean=False, occ_prob=False)[3]
    assert d.tobytes() == d_same.tobytes() and d.tobytes() != d_other.tobytes()
    d_part = ds.abundance_posterior(th[:7], seed=1, log_lik=False, n_mean=False, occ_prob=False)[3]   # (seed, draw, period, site) only
    assert np.array_equal(d_part, d[:7])
    assert d.min() >= 0 and d.max() <= K
    seen = ~(np.isnan(Y[0]) | np.isnan(W).any(-1) | np.isnan(X).any(-1)[:, None, None])
    if model == "nmixture":
        ymax = np.where(seen, np.nan_to_num(Y[0]), 0.0).max(-1).T
        assert ymax.max() >= 3 and np.all(d >= ymax[None])
    else:
        det = ((np.nan_to_num(Y[0]) > 0) & seen).any(-1).T
        assert det.sum() > 50 and np.all(d[:, det] >= 1)
    wide = c["sd"] >= 0.2
    assert wide.sum() >= 200
    score = (d.astype(np.float64).mean(0) - c["mean"])[wide] / (c["sd"][wide] / math.sqrt(n))
    print(f"\n[draws {model}] {wide.sum()} cells with sd >= 0.2: max |score| {np.max(np.abs(score)):.2f}, mean squared score {np.mean(score ** 2):.3f}")
    assert np.max(np.abs(score)) <= 5.0
    assert 0.8 <= np.mean(score ** 2) <= 1.2
    mode = c["pmf"].argmax(-1)                                                  # (T, N)
    off_mass = np.clip(1.0 - c["pmf"].max(-1), 0.0, 1.0)[~wide]
    off = (d != mode[None]).sum(0)[~wide]
    lo_q, hi_q = stats.binom.ppf(1e-7, n, off_mass), stats.binom.isf(1e-7, n, off_mass)
    sure = off_mass < 1e-12
    print(f"[draws {model}] {(~wide).sum()} cells with sd < 0.2 ({sure.sum()} on one value): draws off the mode {off.sum()} (expected {n * off_mass.sum():.1f})")
    assert np.all(off >= lo_q) and np.all(off <= hi_q)
    assert np.all(off[sure] == 0)
    # pooled over all cells: the histogram over n against the summed pmf, bins merged to an expected count >= 20
    obs_n = np.bincount(d.reshape(-1), minlength=K + 1).astype(np.float64)
    exp_n = n * c["pmf"].sum(axis=(0, 1))
    o_b, e_b, oo, ee = [], [], 0.0, 0.0
    for k in range(K + 1):
        oo, ee = oo + obs_n[k], ee + exp_n[k]
        if ee >= 20.0:
            o_b.append(oo)
            e_b.append(ee)
            oo = ee = 0.0
    o_b[-1] += oo
    e_b[-1] += ee
    o_b, e_b = np.array(o_b), np.array(e_b)
    chi2 = float(((o_b - e_b) ** 2 / e_b).sum())
    crit = float(stats.chi2.ppf(0.999, len(e_b) - 1))
    print(f"[draws {model}] pooled chi-square {chi2:.1f} on {len(e_b)} bins (99.9 % point {crit:.1f})")
    assert len(e_b) >= 5 and chi2 <= crit
    ds.close()


def test_chunk_boundary():
    N, n, K = 20000, 4000, 20   # each output: 320 MB, more than one 256 MB chunk of device scratch
    rng = np.random.default_rng(3)
    X, W = rng.normal(size=(N, 1)), rng.normal(size=(N, 1, 3, 1))
    Y = (rng.uniform(size=(1, N, 1, 3)) < 0.2).astype(np.float64)
    Y[rng.uniform(size=Y.shape) < 0.2] = np.nan
    th = rng.uniform(-1.5, 1.5, size=(n, 4)).astype(np.float32)
    ds = OccuDataset(X, W, Y, model="occu_rn", max_abundance=K)
    ll, mean, _, draw = ds.abundance_posterior(th, seed=9, occ_prob=False)
    assert ll.nbytes > (256 << 20)
    worst = 0.0
    for b in (0, 1, 3354, 3355, n - 2, n - 1):   # both sides of the boundary (3355 draws of 80 kB fill a chunk), first and last draw
        c = A.rn_cells(X, W, Y[0], th[b].astype(np.float64), K)
        bl, bm, _ = A.bounds(c, 1e-5)
        cells = np.random.default_rng(b).choice(N, size=2000, replace=False)
        el, em = np.abs(ll[b][:, cells] - c["l"][:, cells]), np.abs(mean[b][:, cells] - c["mean"][:, cells])
        worst = max(worst, float(np.max(el / bl[:, cells])), float(np.max(em / bm[:, cells])))
        assert np.all(el <= bl[:, cells]) and np.all(em <= bm[:, cells]), b
        assert np.all(c["pmf"][0, cells, draw[b][0, cells]] > 0)
    assert draw.min() >= 0 and draw.max() <= K
    tail = ds.abundance_posterior(th[:3], seed=9, log_lik=False, n_mean=False, occ_prob=False)[3]
    assert np.array_equal(tail, draw[:3])
    # a shorter call that still crosses the boundary, with fewer outputs: the others do not change, bit for bit, on both sides
    ll2, _, _, draw2 = ds.abundance_posterior(th[:3400], seed=9, n_mean=False, occ_prob=False)
    assert np.array_equal(ll2, ll[:3400]) and np.array_equal(draw2, draw[:3400])
    print(f"\n[chunks] max error / bound on the sampled cells: {worst:.3f}")
    ds.close()


def test_abi_refusals_busy_and_optional_outputs():
    data, _, _ = quiet_simulate(n_sites=60, deployment_days_per_site=28, random_seed=1)
    X, W, Y = data["site_covs"], data["obs_covs"], data["obs"]
    cnt = np.nan_to_num(Y) * 2
    comb = _sim(simulate_comb, n_sites=40, random_seed=1)[0]
    handles = [("occu", OccuDataset(X, W, Y)), ("occu with false positives", OccuDataset(X, W, Y, model="occu_fp", fp_mode="constant")),
               ("occu with random effects", OccuDataset(X, W, Y, model="occu_re", site_random_effects=True)),
               ("occu_cop", OccuDataset(X, W, cnt, model="occu_cop", fp_mode=None, session_duration=np.ones(Y.shape[1:]))),
               ("occu_cs", OccuDataset(X, W, np.where(np.isnan(Y), np.nan, Y * 2.0 - 1.0), model="occu_cs")), ("occu_dyn", OccuDataset(X, W, Y, model="occu_dyn")),
               ("joint-species", OccuDataset(X, W, np.concatenate([Y, Y]))),
               ("occu_cop", OccuDataset(X, W, cnt, model="occu_cop", fp_mode=None, session_duration=np.ones(Y.shape[1:]), site_random_effects=True)),
               ("occu_cop", OccuDataset(X, W, cnt, model="occu_cop", fp_mode="constant", session_duration=np.ones(Y.shape[1:]), obs_random_effects=True)),
               ("occu_comb", OccuDataset(comb["site_covs"], comb["PC_obs_covs"], comb["PC_obs"][:1], model="occu_comb", ARU_obs_covs=comb["ARU_obs_covs"],
                                         ARU_obs=comb["ARU_obs"][:1], scores_obs=comb["scores_obs"][:1]))]
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    for name, ds in handles:
        dr = np.zeros((2, ds.D), dtype=np.float32)
        out = np.zeros((2, ds.T, ds.N), dtype=np.float32)
        assert ds._lib.bl_abundance_posterior(ds._h, 2, fp(dr), 0, fp(out), None, None, None) == _ffi.BL_ERR_UNSUPPORTED, name
        assert name in ds._lib.bl_last_error().decode(), (name, ds._lib.bl_last_error())
        with pytest.raises(NotImplementedError):
            ds.abundance_posterior(dr)
        ds.close()
    ds = OccuDataset(X, W, Y, model="occu_rn", max_abundance=20)
    dr = np.random.default_rng(0).uniform(-1, 1, size=(3, ds.D)).astype(np.float32)
    out = np.zeros((3, ds.T, ds.N), dtype=np.float32)
    assert ds._lib.bl_abundance_posterior(ds._h, 0, fp(dr), 0, fp(out), None, None, None) == _ffi.BL_ERR_INVALID
    assert ds._lib.bl_abundance_posterior(ds._h, 3, fp(dr), 0, None, None, None, None) == _ffi.BL_ERR_INVALID
    assert ds._lib.bl_abundance_posterior(ds._h, 3, None, 0, fp(out), None, None, None) == _ffi.BL_ERR_INVALID
    full = ds.abundance_posterior(dr, seed=3)
    for k in range(4):   # every output alone equals its part of the full call
        only = ds.abundance_posterior(dr, seed=3, **{name: i == k for i, name in enumerate(("log_lik", "n_mean", "occ_prob", "n_draw"))})
        assert [o is None for o in only] == [i != k for i in range(4)] and np.array_equal(only[k], full[k])
    # the existing entries keep their refusals on the handles this entry serves
    dn = OccuDataset(X, W, cnt, model="nmixture", max_abundance=20)
    u8, i32 = np.zeros((3, ds.T, ds.N), dtype=np.uint8), np.zeros((3, ds.T, ds.N), dtype=np.int32)
    pu8, pi32 = u8.ctypes.data_as(C.POINTER(C.c_uint8)), i32.ctypes.data_as(C.POINTER(C.c_int32))
    for h in (ds, dn):
        with pytest.raises(NotImplementedError):
            h.site_posterior(dr)
        assert h._lib.bl_site_posterior(h._h, 3, fp(dr), 0, fp(out), None, None) == _ffi.BL_ERR_UNSUPPORTED
        assert h._lib.bl_predict_scores(h._h, 3, fp(dr), 0, pu8, None, None) == _ffi.BL_ERR_UNSUPPORTED
    assert ds._lib.bl_predict_counts(ds._h, 3, fp(dr), 0, pi32, None) == _ffi.BL_ERR_UNSUPPORTED       # occu_rn's sites are not counts
    assert dn._lib.bl_predict(dn._h, 3, fp(dr), 0, pu8, None) == _ffi.BL_ERR_UNSUPPORTED              # nmixture's are
    assert ds.predictive(dr, y=False)[0].shape == dn.predictive(dr, y=False)[0].shape == (3, ds.T, ds.N)   # ... and still serve their own
    dn.close()
    big = _sim(simulate_rn, n_sites=3000, n_site_covs=2, n_obs_covs=2, deployment_days_per_site=70)[0]
    db = OccuDataset(big["site_covs"], big["obs_covs"], big["obs"], model="occu_rn", max_abundance=100)
    db.launch(num_warmup=200000, num_samples=200000, num_chains=2, seed=0)
    time.sleep(0.2)
    assert not db.done()
    with pytest.raises(_ffi.EngineError) as ei:
        db.abundance_posterior(np.zeros((1, db.D), dtype=np.float32))
    assert ei.value.code == _ffi.BL_ERR_BUSY
    db.abort()
    with pytest.raises(Exception, match="aborted"):
        db.wait()
    assert db.abundance_posterior(np.zeros((1, db.D), dtype=np.float32))[0].shape == (1, db.T, db.N)   # the handle stays usable
    db.close()
    ds.close()


def _end_to_end(model_fn, data, truth, n, tag):
    res = fit(model_fn, **data, num_chains=2, num_warmup=300, num_samples=n // 2)
    lat = conditional_abundance(model_fn, res.mcmc, **data, random_seed=4)
    X, W, Y = (np.asarray(data[k], dtype=np.float64) for k in ("site_covs", "obs_covs", "obs"))
    N, T = W.shape[0], W.shape[1]
    assert list(lat) == ["abundance", "N_mean", "occ_prob", "N_i", "log_lik", "n_obs"]
    for k, dt in (("abundance", np.float32), ("N_mean", np.float32), ("occ_prob", np.float32), ("N_i", np.int32), ("log_lik", np.float32)):
        assert lat[k].shape == (n, T, N, 1) and lat[k].dtype == dt, k
    assert lat["n_obs"].shape == (T, N, 1) and lat["n_obs"].dtype == np.int32
    np.testing.assert_allclose(lat["abundance"], res.samples["abundance"], rtol=0, atol=0)
    w = waic_marginal(lat)
    assert all(np.isfinite(v) for v in w.values()) and w["p_waic"] > 0
    col = np.asarray(lat["log_lik"], dtype=np.float64)[:, lat["n_obs"] > 0]
    hand = float(np.sum(np.logaddexp.reduce(col, axis=0) - math.log(n)))
    assert abs(lppd_marginal(lat) - hand) <= 1e-10 * abs(hand)
    seen = ~(np.isnan(Y[0]) | np.isnan(W).any(-1) | np.isnan(X).any(-1)[:, None, None])   # a masked visit's y does not count
    det = ((np.nan_to_num(Y[0]) > 0) & seen).any(-1).T                                   # (T, N)
    assert det.sum() > 20
    assert np.all(lat["occ_prob"][:, det, 0] > 0.99) and np.all(lat["N_i"][:, det, 0] >= 1)
    fs = finite_sample_abundance(lat)
    assert fs.shape == (n, T, 1) and np.all(fs >= det.sum(1)[None, :, None])
    if "N_i" in truth:   # the simulator kept the latent abundance: conditioning on the counts must not lose information about it
        Nt = np.asarray(truth["N_i"], dtype=np.float64)[0].reshape(-1)                   # (S, T, N)
        r_post = np.corrcoef(lat["N_mean"].mean(0)[..., 0].reshape(-1), Nt)[0, 1]
        r_prior = np.corrcoef(lat["abundance"].mean(0)[..., 0].reshape(-1), Nt)[0, 1]
        print(f"\n[{tag} e2e] correlation with the true abundance: N_mean {r_post:.4f}, prior abundance {r_prior:.4f}")
        assert r_post >= r_prior
    return res, lat


def test_end_to_end_rn():
    # (simulate_rn's truth holds lambda, not the latent N: the check that conditioning helps runs for nmixture only)
    data, truth = _sim(simulate_rn)
    _end_to_end(occu_rn, data, truth, 500, "occu_rn")


def test_end_to_end_nmixture():
    data, truth = _sim(simulate_nmixture)
    res, lat = _end_to_end(nmixture, data, truth, 500, "nmixture")
    preds = predict(nmixture, res.mcmc, **data, num_samples=500)
    assert preds["N_i"].shape == lat["N_i"].shape   # the conditional draw carries predict()'s name and shape


def test_occu_and_occu_rn_compare_on_the_same_detections():
    data, _ = _sim(simulate_rn, n_sites=200, deployment_days_per_site=70, simulate_missing=True, random_seed=2)
    kw = dict(num_chains=2, num_warmup=300, num_samples=200)
    a = conditional_occupancy(occu, fit(occu, **data, **kw).mcmc, **data)
    b = conditional_abundance(occu_rn, fit(occu_rn, **data, **kw).mcmc, **data)
    assert np.array_equal(a["n_obs"], b["n_obs"]) and a["log_lik"].shape == b["log_lik"].shape
    wa, wb = waic_marginal(a), waic_marginal(b)
    print(f"\n[waic] occu {wa['waic']:.2f}, occu_rn {wb['waic']:.2f}")
    assert all(np.isfinite(v) for v in wa.values()) and all(np.isfinite(v) for v in wb.values())
