"""bl_path_posterior on the device against the float64 restatement in tests/dyn_path_ref.py: per-element parity of the site
log-likelihood, the smoothed marginals and the pairwise terms at random theta, the exact structure (sites without data, seasons with a
detection), the sum identity with the sampler's own density on the same handle, T = 1 against bl_site_posterior, the joint draws
(seeded, chunk-independent, calibrated marginally AND pairwise), the chunk boundary, the refusals, and fit -> conditional_dynamics end
to end.

Bounds (tests/dyn_path_ref.py: bounds): |l32 - l64| <= rtol S + ulp32(l64) / 2 with S the sum over the site's seasons of |visit terms| +
|kb_t| + |log pi_t| + |log(1 - pi_t)| and rtol = 1e-6, the bound test_gpu_dyn.py commits for this model's bl_logp_grad; z_prob, col_prob,
ext_prob: half of that + 2^-23.  tests/test_dynamics_cpu.py shows in float32 NumPy that the recursions as the kernel writes them stay
below 0.11 of every bound at every case used here.  Every check prints the largest measured error as a fraction of its bound
(pytest -s).  Measured on an MI355X, largest over the 24 parity cases as error / bound: log_lik 0.084, z_prob 0.095, col_prob 0.052,
ext_prob 0.033, sum identity 0.533; T = 1 against bl_site_posterior 0.045 of the two kernels' summed bounds; the chunk-boundary sample
0.057.  Draws: 2 331 261 cells and 1 553 167 pairs in range, standardised sums 1.90 (z - z_prob) and -1.84 (1[colonised] - col_prob),
bound 4.5.  End to end: Brier score 0.056 against 0.226 for the propagated prior."""
import contextlib
import ctypes as C
import io
import time

import numpy as np
import pytest
from scipy import stats

import dyn_path_ref as R
import latent_ref as L
from biolith_amd import _ffi
from biolith_amd.engine import OccuDataset
from biolith_amd.evaluation import finite_sample_occupancy, finite_sample_turnover, waic_marginal
from biolith_amd.models import occu_dyn, simulate_dyn
from biolith_amd.utils import conditional_dynamics, fit
from conftest import quiet_simulate

pytestmark = pytest.mark.gpu


def _dyn(X, W, Y):
    return OccuDataset(X, W, Y, model="occu_dyn")


@pytest.mark.parametrize("N", R.PARITY_N)
@pytest.mark.parametrize("ks,ko", R.PARITY_K)
@pytest.mark.parametrize("T", R.PARITY_T)
def test_parity_structure_and_sum_identity(T, ks, ko, N):
    X, W, Y, th = R.parity_case(T, ks, ko, N)
    J = W.shape[2]
    ds = _dyn(X, W, Y)
    ll, q, col, ext, z = ds.path_posterior(th, seed=5)
    n = th.shape[0]
    assert ll.shape == (n, N) and q.shape == z.shape == (n, T, N) and col.shape == ext.shape == (n, T - 1, N)
    assert ll.dtype == q.dtype == col.dtype == ext.dtype == np.float32 and z.dtype == np.uint8
    assert all(np.all(np.isfinite(a)) for a in (ll, q, col, ext))
    assert all(np.all((a >= 0) & (a <= 1)) for a in (q, col, ext)) and set(np.unique(z)) <= {0, 1}
    U = ds.logp_grad(th)[0]
    m = ~(np.isnan(Y[0]) | np.isnan(W).any(-1) | np.isnan(X).any(-1)[:, None, None])
    det = ((np.nan_to_num(Y[0]) > 0) & m).any(-1).T            # (T, N): a season with an unmasked detection
    assert det.any()
    worst = dict(log_lik=0.0, z_prob=0.0, col_prob=0.0, ext_prob=0.0, sum=0.0)
    for b in range(n):
        c = R.dyn_paths(X, W, Y, th[b])
        bl, bp = R.bounds(c, R.RTOL)
        for name, got, want, bound in (("log_lik", ll[b], c["l"], bl), ("z_prob", q[b], c["q"], bp), ("col_prob", col[b], c["col"], bp),
                                       ("ext_prob", ext[b], c["ext"], bp)):
            frac = float(np.max(np.abs(got - want) / bound, initial=0.0))
            worst[name] = max(worst[name], frac)
            assert frac <= 1.0, (name, b, frac)
        empty = c["n_obs"] == 0
        assert empty.sum() >= 4
        assert np.all(ll[b][empty] == 0.0)           # exactly: nothing observed in any season, likelihood 1
        prior = R.propagated_prior(c["psi"], c["gamma"], c["eps"], T)
        assert np.all(np.abs(q[b][:, empty] - prior[:, empty]) <= bp[empty])
        assert np.all(q[b][det] >= 1 - 2.0 ** -24) and np.all(z[b][det] == 1)     # a detection proves occupancy in that season
        want = -U[b] - float(np.sum(stats.norm.logpdf(th[b])))   # the sites add up to the likelihood part of the sampler's own potential
        got = float(ll[b].astype(np.float64).sum())
        worst["sum"] = max(worst["sum"], abs(got - want) / (R.RTOL * abs(want)))
        assert abs(got - want) <= R.RTOL * abs(want), (b, got, want)
    print(f"\n[dyn T={T} K=({ks},{ko}) N={N} J={J}] max error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    ds.close()


def test_one_season_is_the_static_model():
    X, W, Y, th = R.parity_case(1, 2, 2, 300)
    dyn, occ = _dyn(X, W, Y), OccuDataset(X, W, Y)
    th_occ = np.concatenate([th[:, :3], th[:, 9:]], axis=1)     # [beta | alpha]
    ll, q, col, ext, z = dyn.path_posterior(th, seed=1)
    ll_s, q_s, _ = occ.site_posterior(th_occ, seed=1)
    assert col.shape == ext.shape == (4, 0, 300)
    worst = 0.0
    for b in range(4):
        bl_d, bq_d = R.bounds(R.dyn_paths(X, W, Y, th[b]), R.RTOL)
        bl_s, bq_s = L.bounds(L.occu_cells(X, W, Y[0], th_occ[b]), 1e-6)
        el, eq = np.abs(ll[b] - ll_s[b, 0]) / (bl_d + bl_s[0]), np.abs(q[b, 0] - q_s[b, 0]) / (bq_d + bq_s[0])
        worst = max(worst, float(el.max()), float(eq.max()))
        assert np.all(el <= 1) and np.all(eq <= 1), b
    print(f"\n[dyn T=1 against bl_site_posterior] max difference / (sum of the two bounds): {worst:.3f}")
    dyn.close()
    occ.close()


def test_draws_are_seeded_and_calibrated_jointly():
    N, T, J, n = 4000, 3, 3, 300
    X, W, Y, centre = R.draws_case(N, T, J, seed=11)
    th = (centre + np.random.default_rng(2).normal(scale=0.15, size=(n, centre.size))).astype(np.float32)
    # the restatement's own marginals leave enough cells in range (float64, no device)
    ref = [R.dyn_paths(X, W, Y, t) for t in th.astype(np.float64)]
    q64, c64 = np.stack([c["q"] for c in ref]), np.stack([c["col"] for c in ref])
    assert ((q64 > 0.05) & (q64 < 0.95)).sum() >= 10 ** 5 and ((c64 > 0.02) & (c64 < 0.98)).sum() >= 10 ** 5
    ds = _dyn(X, W, Y)
    _, q, col, _, z = ds.path_posterior(th, seed=1)
    only_z = dict(log_lik=False, z_prob=False, col_prob=False, ext_prob=False)
    z_same, z_other = ds.path_posterior(th, seed=1, **only_z)[4], ds.path_posterior(th, seed=2, **only_z)[4]
    assert z.tobytes() == z_same.tobytes() and z.tobytes() != z_other.tobytes()
    assert np.array_equal(ds.path_posterior(th[:7], seed=1, **only_z)[4], z[:7])   # (seed, draw, period, site) only
    s_q, n_q = R.standardised(z, q, 0.05, 0.95)
    s_c, n_c = R.standardised((z[:, :-1] == 0) & (z[:, 1:] == 1), col, 0.02, 0.98)
    print(f"\n[dyn draws] {n_q} cells / {n_c} pairs in range, standardised sums: z - z_prob {s_q:.3f}, 1[colonised] - col_prob {s_c:.3f}")
    assert n_q >= 10 ** 5 and n_c >= 10 ** 5
    assert abs(s_q) <= 4.5 and abs(s_c) <= 4.5
    ds.close()


def test_chunk_boundary():
    N, T, n = 20000, 2, 2500   # z_prob: 400 MB, more than one 256 MB chunk of device scratch
    rng = np.random.default_rng(3)
    X, W = rng.normal(size=(N, 1)), rng.normal(size=(N, T, 3, 1))
    Y = (rng.uniform(size=(1, N, T, 3)) < 0.2).astype(np.float64)
    Y[rng.uniform(size=Y.shape) < 0.2] = np.nan
    th = rng.uniform(-1.5, 1.5, size=(n, 8)).astype(np.float32)
    ds = _dyn(X, W, Y)
    _, q, _, _, z = ds.path_posterior(th, seed=9, log_lik=False, col_prob=False, ext_prob=False)
    assert q.nbytes > (256 << 20)
    per_chunk = (256 << 20) // (T * N * 4)   # 1677 draws of 160 kB fill a chunk
    assert 1 < per_chunk < n
    worst = 0.0
    for b in (0, per_chunk - 1, per_chunk, n - 1):   # both sides of the boundary, first and last draw
        c = R.dyn_paths(X, W, Y, th[b].astype(np.float64))
        sites = np.random.default_rng(b).choice(N, size=2000, replace=False)
        eq = np.abs(q[b][:, sites] - c["q"][:, sites]) / R.bounds(c, R.RTOL)[1][sites]
        worst = max(worst, float(eq.max()))
        assert np.all(eq <= 1), b
    assert np.array_equal(ds.path_posterior(th[:3], seed=9, log_lik=False, z_prob=False, col_prob=False, ext_prob=False)[4], z[:3])
    print(f"\n[dyn chunks] max error / bound on the sampled sites: {worst:.3f}")
    ds.close()


def test_abi_refusals_and_busy():
    data, _, _ = quiet_simulate(n_sites=60, deployment_days_per_site=28, random_seed=1)
    X, W, Y = data["site_covs"], data["obs_covs"], data["obs"]
    cnt = np.nan_to_num(Y) * 2
    with contextlib.redirect_stdout(io.StringIO()):
        from biolith_amd.models import simulate_comb
        cd, _ = simulate_comb(n_sites=40, random_seed=1)
    handles = [("occu", OccuDataset(X, W, Y)), ("occu_fp", OccuDataset(X, W, Y, model="occu_fp", fp_mode="constant")),
               ("occu_re", OccuDataset(X, W, Y, model="occu_re", site_random_effects=True, obs_random_effects=False)),
               ("occu_rn", OccuDataset(X, W, Y, model="occu_rn", max_abundance=20)), ("nmixture", OccuDataset(X, W, cnt, model="nmixture", max_abundance=20)),
               ("occu_cop", OccuDataset(X, W, cnt, model="occu_cop", fp_mode=None, session_duration=np.ones(Y.shape[1:]))),
               ("occu_cs", OccuDataset(X, W, np.where(np.isnan(Y), np.nan, Y * 2.0 - 1.0), model="occu_cs")),
               ("occu_comb", OccuDataset(cd["site_covs"], cd["PC_obs_covs"], cd["PC_obs"][:1], model="occu_comb", ARU_obs_covs=cd["ARU_obs_covs"],
                                         ARU_obs=cd["ARU_obs"][:1], scores_obs=cd["scores_obs"][:1])),
               ("joint-species", OccuDataset(X, W, np.concatenate([Y, Y])))]
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    for name, ds in handles:
        dr = np.zeros((2, ds.D), dtype=np.float32)
        out = np.zeros((2, ds.N), dtype=np.float32)
        assert ds._lib.bl_path_posterior(ds._h, 2, fp(dr), 0, fp(out), None, None, None, None) == _ffi.BL_ERR_UNSUPPORTED, name
        msg = ds._lib.bl_last_error().decode()
        assert name in msg and "bl_site_posterior" in msg, (name, msg)
        with pytest.raises(NotImplementedError):
            ds.path_posterior(dr)
        ds.close()
    ds = _dyn(X, W, Y)
    assert ds._lib.bl_path_posterior(ds._h, 0, None, 0, None, None, None, None, None) == _ffi.BL_ERR_INVALID
    ds.close()
    with contextlib.redirect_stdout(io.StringIO()):
        big, _ = simulate_dyn(n_sites=2000, n_periods=8, n_site_covs=3, n_obs_covs=3, deployment_days_per_site=28, session_duration=7)
    db = _dyn(big["site_covs"], big["obs_covs"], big["obs"])
    db.launch(num_warmup=200000, num_samples=200000, num_chains=2, seed=0)
    time.sleep(0.2)
    assert not db.done()
    with pytest.raises(_ffi.EngineError) as ei:
        db.path_posterior(np.zeros((1, db.D), dtype=np.float32))
    assert ei.value.code == _ffi.BL_ERR_BUSY
    db.abort()
    with pytest.raises(Exception, match="aborted"):
        db.wait()
    assert db.path_posterior(np.zeros((1, db.D), dtype=np.float32))[1].shape == (1, db.T, db.N)   # the handle stays usable
    db.close()


def test_end_to_end():
    with contextlib.redirect_stdout(io.StringIO()):
        data, truth = simulate_dyn(**R.E2E)
    res = fit(occu_dyn, **data, num_chains=2, num_warmup=300, num_samples=250)
    lat = conditional_dynamics(occu_dyn, res.mcmc, **data, random_seed=4)
    n, T, N = 500, 5, 300
    assert list(lat) == ["psi", "gamma", "epsilon", "z_prob", "z", "col_prob", "ext_prob", "log_lik", "n_obs", "n_obs_period"]
    for k, shape, dt in (("psi", (n, N, 1), np.float32), ("gamma", (n, N, 1), np.float32), ("epsilon", (n, N, 1), np.float32),
                         ("z_prob", (n, T, N, 1), np.float32), ("z", (n, T, N, 1), np.int32), ("col_prob", (n, T - 1, N, 1), np.float32),
                         ("ext_prob", (n, T - 1, N, 1), np.float32), ("log_lik", (n, N, 1), np.float32), ("n_obs", (N, 1), np.int32),
                         ("n_obs_period", (T, N, 1), np.int32)):
        assert lat[k].shape == shape and lat[k].dtype == dt, k
    np.testing.assert_allclose(lat["psi"], res.samples["psi"], rtol=0, atol=0)
    zt = np.asarray(truth["z"], dtype=np.float64)                     # (T, N)
    q = lat["z_prob"].mean(0)[..., 0].astype(np.float64)
    prior = R.propagated_prior(lat["psi"][..., 0].astype(np.float64), lat["gamma"][..., 0].astype(np.float64), lat["epsilon"][..., 0].astype(np.float64), T).mean(0)
    b_q, b_prior = float(np.mean((q - zt) ** 2)), float(np.mean((prior - zt) ** 2))
    turn = finite_sample_turnover(lat)
    col = float(np.nanmean(turn["colonisation"]))
    print(f"\n[dyn e2e] Brier: z_prob {b_q:.4f}, propagated prior {b_prior:.4f}; mean z_prob {q.mean():.4f} (true {zt.mean():.4f}); "
          f"colonisation {col:.4f} (true gamma {truth['gamma'].mean():.4f})")
    assert b_q < b_prior
    assert abs(q.mean() - zt.mean()) < 0.1
    w = waic_marginal(lat)
    assert all(np.isfinite(v) for v in w.values()) and w["p_waic"] > 0
    assert finite_sample_occupancy(lat).shape == (n, T, 1)
    assert turn["colonisation"].shape == turn["extinction"].shape == (n, T - 1, 1)
    assert np.all(np.isfinite(turn["colonisation"])) and np.all(np.isfinite(turn["extinction"]))
    assert abs(col - truth["gamma"].mean()) < 0.15
    X, W, Y = (np.asarray(data[k], dtype=np.float64) for k in ("site_covs", "obs_covs", "obs"))
    seen = ~(np.isnan(Y[0]) | np.isnan(W).any(-1) | np.isnan(X).any(-1)[:, None, None])   # a masked visit's y does not count
    det = ((np.nan_to_num(Y[0]) > 0) & seen).any(-1).T                                     # (T, N)
    assert det.sum() > 200
    assert np.all(lat["z"][:, det, 0] == 1)   # a site-season with a detection is occupied in every conditional path
