"""predict_comb on the GPU: occu_comb's posterior predictive (bl_predict_comb) and deterministic sites (bl_deterministic_comb) against
float64 closed forms, structural identities, exact Bernoulli / Normal moments at 5 sigma, seeding and chunking, empty blocks, missing
covariates, new sites, several species, the refusals, and the evaluation that consumes the result (waic_comb, the predictive check).

Distributions are checked on hand-made "posteriors" (one theta tiled n times); the two fits are small (40 / 30 sites, 100 + 100 draws)."""
import contextlib
import ctypes as C
import io
import math

import numpy as np
import pytest

from biolith_amd import _ffi
from biolith_amd.engine import OccuDataset
from biolith_amd.evaluation import posterior_predictive_check, residuals, waic_comb
from biolith_amd.models import occu_comb, simulate, simulate_comb
from biolith_amd.utils import fit, predict_comb

pytestmark = pytest.mark.gpu

RATES = ("ARU_prob_fp_constant", "ARU_fp_unoccupied", "mu0", "mu1", "sigma0", "sigma1")
KEYS = {"psi", "z", "PC_prob_detection", "ARU_prob_detection", "ARU_prob_detection_fp", "y_pc", "y_aru", "scores", *RATES}
COVS = ("site_covs", "PC_obs_covs", "ARU_obs_covs")


def _data(**kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return simulate_comb(**kw)


class _Posterior:
    """What predict_comb reads of a fit: ``get_samples()``."""

    def __init__(self, sites):
        self.sites = sites

    def get_samples(self):
        return self.sites


def _tiled(n, beta, alpha_pc, alpha_aru, fc=0.1, fu=0.2, mu0=-3.0, mu1=2.0, sigma0=5.0, sigma1=3.0):
    """One theta, n times, one species."""
    f32 = lambda a: np.tile(np.asarray(a, dtype=np.float32)[None, None], (n, 1) + (1,) * np.ndim(a))
    sites = dict(beta=f32(beta), alpha_PC=f32(alpha_pc), alpha_ARU=f32(alpha_aru))
    for k, v in zip(RATES, (fc, fu, mu0, mu1, sigma0, sigma1)):
        sites[k] = np.full((n, 1), v, dtype=np.float32)
    return _Posterior(sites)


def _covs(rng, N, T, Jpc, Jaru, Ks, Kpc, Karu):
    return dict(site_covs=rng.normal(size=(N, Ks)), PC_obs_covs=rng.normal(size=(N, T, Jpc, Kpc)), ARU_obs_covs=rng.normal(size=(N, T, Jaru, Karu)))


def _closed(posterior, covs, sp=0):
    """float64 closed forms on the posterior's own (float32) draws: psi (n, T, N), p_pc (n, Jpc, T, N), p_aru (n, Jaru, T, N)."""
    X, Wp, Wa = (np.nan_to_num(np.asarray(covs[k], dtype=np.float32)).astype(np.float64) for k in COVS)
    b, ap, aa = (np.asarray(posterior[k], dtype=np.float64)[:, sp] for k in ("beta", "alpha_PC", "alpha_ARU"))
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    psi = sig(b[:, :1] + b[:, 1:] @ X.T)                                                       # (n, N)
    det = lambda a, W: sig(a[:, 0][:, None, None, None] + np.einsum("itjk,nk->njti", W, a[:, 1:]))
    return np.broadcast_to(psi[:, None], (psi.shape[0], Wp.shape[1], psi.shape[1])), det(ap, Wp), det(aa, Wa)


def _within(total, mean, var, what):
    assert abs(total - mean) <= 5.0 * math.sqrt(var) + 1e-9, (what, total, mean, math.sqrt(var))


def _check_moments(preds, posterior, covs):
    """5 sigma: the Bernoulli sums given the realised z (exact means and variances), the scores' means and variances by z."""
    psi, ppc, paru = _closed(posterior, covs)
    z = preds["z"][..., 0].astype(np.float64)
    _within(z.sum(), psi.sum(), (psi * (1 - psi)).sum(), "z")
    p = z[:, None] * ppc
    _within(preds["y_pc"].sum(), p.sum(), (p * (1 - p)).sum(), "y_pc")
    fc, fu = (np.asarray(posterior[k], dtype=np.float64).reshape(-1, 1, 1, 1) for k in RATES[:2])
    p = 1 - (1 - z[:, None] * paru) * (1 - fc) * (1 - (1 - z[:, None]) * fu)
    _within(preds["y_aru"].sum(), p.sum(), (p * (1 - p)).sum(), "y_aru")
    s = preds["scores"][..., 0].astype(np.float64)
    if s.shape[1]:
        zz = np.broadcast_to(z[:, None], s.shape)
        for state, mu, sg in ((0, "mu0", "sigma0"), (1, "mu1", "sigma1")):
            g, mu, sg = s[zz == state], float(posterior[mu][0, 0]), float(posterior[sg][0, 0])
            assert g.size > 1000
            assert abs(g.mean() - mu) <= 5 * sg / math.sqrt(g.size), (state, g.mean(), mu)
            assert abs(g.var(ddof=1) / sg ** 2 - 1) <= 5 * math.sqrt(2 / (g.size - 1)), (state, g.var(ddof=1), sg ** 2)


# ------------------------------------------------------------------------------------------ a small fit, shared ----
@pytest.fixture(scope="module")
def fitted():
    data, _ = _data(n_sites=40, n_periods=2, PC_replicates=3, ARU_replicates=5, scores_replicates=4, n_site_covs=2, n_PC_covs=1, n_ARU_covs=2,
                    ARU_prob_fp_constant=0.05, ARU_prob_fp_unoccupied=0.1, simulate_missing=True, random_seed=3)
    res = fit(occu_comb, **data, num_chains=2, num_samples=100, num_warmup=100, timeout=600)
    return data, res, predict_comb(occu_comb, res.mcmc, **data)


def test_deterministic_sites_of_a_fit(fitted):
    data, res, preds = fitted
    post = res.mcmc.get_samples()
    n, T, N, S, Jpc, Jaru, Js = 200, 2, 40, 1, 3, 5, 4
    assert set(preds.keys()) == KEYS
    shapes = dict(psi=(n, T, N, S), z=(n, T, N, S), PC_prob_detection=(n, Jpc, T, N, S), ARU_prob_detection=(n, Jaru, T, N, S),
                  ARU_prob_detection_fp=(n, Jaru, T, N, S), y_pc=(n, Jpc, T, N, S), y_aru=(n, Jaru, T, N, S), scores=(n, Js, T, N, S))
    for k, shape in shapes.items():
        assert preds[k].shape == shape, k
        assert preds[k].dtype == (np.int32 if k in ("z", "y_pc", "y_aru") else np.float32), k
    for k in RATES:
        assert preds[k].shape == (n, S) and preds[k].dtype == np.float32 and np.array_equal(preds[k], np.asarray(post[k], np.float32).reshape(n, S))
    assert set(np.unique(preds["z"])) <= {0, 1} and set(np.unique(preds["y_pc"])) <= {0, 1} and set(np.unique(preds["y_aru"])) <= {0, 1}
    assert np.all(np.isfinite(preds["scores"])) and np.all(preds["y_pc"] <= preds["z"][:, None])   # no false positives in the point counts
    # the float64 closed form on the posterior draws: bl_deterministic's bound (tests/test_gpu_predict.py), the same __expf sigmoid
    for key, want in zip(("psi", "PC_prob_detection", "ARU_prob_detection"), _closed(post, data)):
        np.testing.assert_allclose(preds[key][..., 0], want, rtol=2e-5, atol=2e-6, err_msg=key)
        # ... and the sites fit() formed on the host in float32 NumPy
        np.testing.assert_allclose(preds[key], np.asarray(res.samples[key]).reshape(preds[key].shape), rtol=2e-5, atol=2e-6, err_msg=key)
    # ARU_prob_detection_fp at the sampled z
    z = preds["z"][:, None].astype(np.float64)
    fc, fu = (preds[k].astype(np.float64)[:, None, None, None, :] for k in RATES[:2])
    want = 1 - (1 - z * preds["ARU_prob_detection"].astype(np.float64)) * (1 - fc) * (1 - (1 - z) * fu)
    np.testing.assert_allclose(preds["ARU_prob_detection_fp"], want, rtol=1e-6, atol=1e-7)


def test_waic_and_predictive_check_of_a_fit(fitted):
    data, _, preds = fitted
    w = waic_comb(preds, **data)
    assert all(math.isfinite(w[k]) for k in ("waic", "p_waic", "lppd")) and w["p_waic"] > 0
    # the point counts are the false-positive-free block the check and the residuals are valid for
    pc = {"psi": preds["psi"], "prob_detection": preds["PC_prob_detection"], "y": preds["y_pc"], "z": preds["z"]}
    for group_by in ("site", "revisit"):
        assert 0.0 <= posterior_predictive_check(pc, data["PC_obs"], group_by=group_by) <= 1.0
    occ, det = residuals(pc, data["PC_obs"])
    assert occ.shape == preds["z"].shape and det.shape == (200, 1, 40, 2, 3)


def test_new_sites_and_wrong_covariate_counts(fitted):
    _, res, _ = fitted
    new, _ = _data(n_sites=23, n_periods=3, PC_replicates=2, ARU_replicates=4, scores_replicates=2, n_site_covs=2, n_PC_covs=1, n_ARU_covs=2,
                   random_seed=9)
    covs = {k: new[k] for k in COVS}
    preds = predict_comb(occu_comb, res.mcmc, **covs, scores_replicates=6, random_seed=4)
    assert preds["z"].shape == (200, 3, 23, 1) and preds["y_pc"].shape == (200, 2, 3, 23, 1) and preds["y_aru"].shape == (200, 4, 3, 23, 1)
    assert preds["scores"].shape == (200, 6, 3, 23, 1)
    for key, want in zip(("psi", "PC_prob_detection", "ARU_prob_detection"), _closed(res.mcmc.get_samples(), covs)):
        np.testing.assert_allclose(preds[key][..., 0], want, rtol=2e-5, atol=2e-6, err_msg=key)
    for k in COVS:   # one covariate too many in each block in turn
        bad = dict(covs, **{k: np.concatenate([covs[k], covs[k][..., :1]], axis=-1)})
        with pytest.raises(ValueError, match="covariate counts"):
            predict_comb(occu_comb, res.mcmc, **bad, scores_replicates=2)
    with pytest.raises(ValueError, match="scores_obs or scores_replicates"):
        predict_comb(occu_comb, res.mcmc, **covs)
    with pytest.raises(ValueError, match="species"):
        predict_comb(occu_comb, res.mcmc, **covs, scores_obs=np.zeros((2, 23, 3, 2)))


def test_two_species():
    data, _ = _data(n_species=2, n_sites=30, simulate_missing=True, random_seed=5)
    res = fit(occu_comb, **data, num_chains=1, num_samples=100, num_warmup=100, timeout=600)
    preds = predict_comb(occu_comb, res.mcmc, **data)
    post = res.mcmc.get_samples()
    assert preds["psi"].shape == (100, 1, 30, 2) and preds["y_aru"].shape == (100, 24, 1, 30, 2) and preds["mu0"].shape == (100, 2)
    for sp in range(2):
        for key, want in zip(("psi", "PC_prob_detection", "ARU_prob_detection"), _closed(post, data, sp)):
            np.testing.assert_allclose(preds[key][..., sp], want, rtol=2e-5, atol=2e-6, err_msg=f"{key}[{sp}]")
    assert not np.array_equal(preds["z"][..., 0], preds["z"][..., 1])
    assert math.isfinite(waic_comb(preds, **data)["waic"])


# ------------------------------------------------------------------------------------------ hand-made posteriors ----
def test_structural_identities():
    rng = np.random.default_rng(0)
    covs = _covs(rng, N=50, T=2, Jpc=3, Jaru=4, Ks=1, Kpc=1, Karu=1)
    # neither false-positive rate: nothing is heard at an unoccupied site, and the rate-free form is z p exactly
    preds = predict_comb(occu_comb, _tiled(300, [0.0, 0.5], [0.3, -0.4], [0.2, 0.6], fc=0.0, fu=0.0), **covs, scores_replicates=2)
    z = preds["z"][:, None]
    assert 0.3 < z.mean() < 0.7
    assert np.all(preds["y_pc"][np.broadcast_to(z == 0, preds["y_pc"].shape)] == 0)
    assert np.all(preds["y_aru"][np.broadcast_to(z == 0, preds["y_aru"].shape)] == 0)
    assert preds["y_pc"].sum() > 0 and preds["y_aru"].sum() > 0
    assert np.array_equal(preds["ARU_prob_detection_fp"], preds["ARU_prob_detection"] * z.astype(np.float32))
    # an unoccupied site always sounds occupied with fu = 1
    preds = predict_comb(occu_comb, _tiled(300, [0.0, 0.5], [0.3, -0.4], [0.2, 0.6], fc=0.0, fu=1.0), **covs, scores_replicates=2)
    z0 = np.broadcast_to(preds["z"][:, None] == 0, preds["y_aru"].shape)
    assert z0.any() and np.all(preds["y_aru"][z0] == 1) and not np.all(preds["y_aru"][~z0] == 1)
    assert np.all(preds["y_pc"][np.broadcast_to(preds["z"][:, None] == 0, preds["y_pc"].shape)] == 0)


def test_distributions():
    # the blocks differ in every dimension and the ARU block has no covariates
    n, N, T = 4000, 37, 3
    covs = _covs(np.random.default_rng(1), N=N, T=T, Jpc=3, Jaru=5, Ks=1, Kpc=2, Karu=0)
    posterior = _tiled(n, [0.1, 0.3], [-0.2, 0.7, -0.5], [0.4])
    preds = predict_comb(occu_comb, posterior, **covs, scores_replicates=4, random_seed=11)
    assert preds["scores"].shape == (n, 4, T, N, 1) and preds["ARU_prob_detection"].shape == (n, 5, T, N, 1)
    _check_moments(preds, posterior.sites, covs)
    psi = _closed(posterior.sites, covs)[0][0]                                                   # (T, N)
    assert np.max(np.abs(preds["z"][..., 0].mean(axis=0) - psi)) <= 5 * math.sqrt(0.25 / n)


@pytest.mark.parametrize("empty", ["PC", "ARU", "scores"])
def test_an_empty_block(empty):
    n, N, T = 1500, 21, 2
    J = {**dict(PC=3, ARU=4, scores=3), empty: 0}
    covs = _covs(np.random.default_rng(2), N=N, T=T, Jpc=J["PC"], Jaru=J["ARU"], Ks=2, Kpc=1, Karu=1)
    posterior = _tiled(n, [0.2, -0.3, 0.4], [0.1, 0.5], [-0.3, 0.4])
    preds = predict_comb(occu_comb, posterior, **covs, scores_replicates=J["scores"], random_seed=2)
    assert preds["y_pc"].shape == (n, J["PC"], T, N, 1) and preds["PC_prob_detection"].shape == (n, J["PC"], T, N, 1)
    assert preds["y_aru"].shape == (n, J["ARU"], T, N, 1) and preds["ARU_prob_detection_fp"].shape == (n, J["ARU"], T, N, 1)
    assert preds["scores"].shape == (n, J["scores"], T, N, 1) and preds["z"].shape == (n, T, N, 1)
    _check_moments(preds, posterior.sites, covs)


def test_missing_covariates_read_as_zero():
    rng = np.random.default_rng(3)
    covs = _covs(rng, N=30, T=2, Jpc=2, Jaru=3, Ks=2, Kpc=1, Karu=2)
    holes = {k: v.copy() for k, v in covs.items()}
    holes["site_covs"][4, 1] = holes["ARU_obs_covs"][7, 1, 2, 0] = holes["PC_obs_covs"][9, 0, 1, 0] = np.nan
    posterior = _tiled(50, [0.2, -0.3, 0.4], [0.1, 0.5], [-0.3, 0.4, 0.8])
    a = predict_comb(occu_comb, posterior, **holes, scores_replicates=2, random_seed=5)
    b = predict_comb(occu_comb, posterior, **{k: np.nan_to_num(v) for k, v in holes.items()}, scores_replicates=2, random_seed=5)
    c = predict_comb(occu_comb, posterior, **covs, scores_replicates=2, random_seed=5)
    for k in KEYS:
        assert np.all(np.isfinite(a[k])), k
        assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a["psi"], c["psi"]) and not np.array_equal(a["ARU_prob_detection"], c["ARU_prob_detection"])


# ------------------------------------------------------------------------------------------ the engine: seeding, chunking ----
def _handle(rng, N, T=2, Jpc=2, Jaru=3, Js=2, Ks=1, Kpc=1, Karu=1):
    c = _covs(rng, N, T, Jpc, Jaru, Ks, Kpc, Karu)
    blank = lambda J: np.full((1, N, T, J), np.nan, dtype=np.float32)
    ds = OccuDataset(c["site_covs"], c["PC_obs_covs"], blank(Jpc), model="occu_comb", ARU_obs_covs=c["ARU_obs_covs"], ARU_obs=blank(Jaru),
                     scores_obs=blank(Js))
    return ds, c


def _draws(rng, n, D):
    th = rng.uniform(-1, 1, size=(n, D))
    th[:, -6:] = np.array([-1.5, -1.0, -3.0, math.log(5.0), math.log(5.0), math.log(3.0)]) + rng.uniform(-0.2, 0.2, size=(n, 6))
    return th.astype(np.float32)


def test_seeding_and_output_selection():
    rng = np.random.default_rng(4)
    ds, _ = _handle(rng, N=300)   # two 256-thread blocks, the second partial
    th = _draws(rng, 40, ds.D)
    a, b, c = ds.predictive_comb(th, seed=7), ds.predictive_comb(th, seed=7), ds.predictive_comb(th, seed=8)
    assert [x.shape for x in a] == [(40, 2, 300), (40, 2, 2, 300), (40, 3, 2, 300), (40, 2, 2, 300)]
    assert [x.dtype for x in a] == [np.uint8, np.uint8, np.uint8, np.float32]
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not np.array_equal(a[0], c[0])
    # the sample is a function of (seed, draw, period, site): the first draws of a longer call are the shorter call
    for x, y in zip(a, ds.predictive_comb(th[:7], seed=7)):
        assert np.array_equal(x[:7], y)
    # no output depends on which others are asked for
    only = ds.predictive_comb(th, seed=7, z=False, y_pc=False, y_aru=False)
    assert only[:3] == (None, None, None) and np.array_equal(only[3], a[3])
    only = ds.predictive_comb(th, seed=7, z=False, y_pc=False, scores=False)
    assert np.array_equal(only[2], a[2])
    only = ds.predictive_comb(th, seed=7, y_aru=False, scores=False)
    assert np.array_equal(only[0], a[0]) and np.array_equal(only[1], a[1])
    psi, ppc, paru = ds.deterministic_comb(th)
    assert ds.deterministic_comb(th, pc_prob=False, aru_prob=False)[1:] == (None, None)
    assert np.array_equal(ds.deterministic_comb(th, psi=False, pc_prob=False)[2], paru)
    ds.close()


def test_more_draws_than_grid_rows():
    rng = np.random.default_rng(5)
    ds, covs = _handle(rng, N=5)
    th = _draws(rng, 1100, ds.D)   # the draw loop strides past grid_y = 1024
    full, head = ds.predictive_comb(th, seed=3), ds.predictive_comb(th[:1024], seed=3)
    for x, y in zip(full, head):
        assert np.array_equal(x[:1024], y)
    assert ds.D == 12
    post = dict(beta=th[:, None, :2], alpha_PC=th[:, None, 2:4], alpha_ARU=th[:, None, 4:6])
    for got, want in zip(ds.deterministic_comb(th), _closed(post, covs)):   # every draw, the 76 of the second stride included
        np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-6)
    z, ypc, yaru, s = full
    tail = slice(1024, None)
    assert np.all(ypc[tail] <= z[tail, None]) and 0.2 < z[tail].mean() < 0.8 and np.all(np.isfinite(s[tail])) and s[tail].std() > 1.0
    ds.close()


def test_other_handles_are_refused():
    with contextlib.redirect_stdout(io.StringIO()):
        data, _ = simulate(n_sites=20, random_seed=0)
    ds = OccuDataset(data["site_covs"], data["obs_covs"], data["obs"])
    lib, n = ds._lib, 2
    dr = np.zeros((n, ds.D), dtype=np.float32)
    fp = dr.ctypes.data_as(C.POINTER(C.c_float))
    u8 = np.zeros(n * ds.T * ds.N * max(ds.J, 1), dtype=np.uint8)
    pu8 = u8.ctypes.data_as(C.POINTER(C.c_uint8))
    out = np.zeros(u8.size, dtype=np.float32)
    po = out.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.bl_predict_comb(ds._h, n, fp, 0, pu8, pu8, pu8, po) == _ffi.BL_ERR_UNSUPPORTED
    assert b"occu" in lib.bl_last_error() and b"bl_predict_comb" in lib.bl_last_error()
    assert lib.bl_deterministic_comb(ds._h, n, fp, po, po, po) == _ffi.BL_ERR_UNSUPPORTED
    assert b"occu" in lib.bl_last_error() and b"bl_deterministic_comb" in lib.bl_last_error()
    assert not u8.any() and not out.any()
    with pytest.raises(NotImplementedError, match="occu"):
        ds.predictive_comb(dr)
    ds.close()
