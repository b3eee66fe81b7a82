"""conditional_counts without a device: the float64 restatement (tests/counts_ref.py) pinned to the potentials the reference's own
occu_cop produced (tests/golden/reference_logjoint_cop_*.json), its structure, expected_true_detections by hand, the Python refusals,
the declarations of the entry, and the draw-frequency criterion of tests/test_gpu_counts.py met by the restatement alone.

The frequency case (counts_ref.frequency_case) has 1086 cells with q in (0.05, 0.95) and 4685 unmasked visits with a positive count and
q rho_j in (0.05, 0.95) -- figures of the restatement, the same for every run; both files require at least 1000 and 4500."""
import os

import numpy as np
import pytest

import counts_ref as R
import reference_logjoint as RL
from biolith_amd import _ffi, models, utils
from biolith_amd.evaluation import expected_true_detections, finite_sample_occupancy, lppd_marginal, waic_marginal
from biolith_amd.utils import conditional_abundance, conditional_counts, conditional_dynamics, conditional_occupancy, conditional_scores
from biolith_amd.utils._conditional import SERVED_BY
from biolith_amd.utils.mcmc import LazySamples

COP_CASES = ["cop_default", "cop_missing", "cop_small_2x2", "cop_fp_constant", "cop_fp_unoccupied", "priors_cop", "cop_re_both"]
MIN_Z_CELLS, MIN_T_VISITS = 1000, 4500   # (module docstring)


@pytest.mark.parametrize("case", COP_CASES)
def test_restatement_sums_to_the_reference_models_likelihood(case):
    """sum over cells of l = -U_fixture - log prior(theta): the priors and the Jacobians of log rate / log sd restated with scipy.stats."""
    e = RL.load(case)
    assert e["model"] == "occu_cop" and e["dims"]["S"] == 1
    X, W, Y, kw = RL.build(e)
    N, T, J, Ko = W.shape
    Ks = X.shape[1]
    site, obs = kw["site_random_effects"], kw["obs_random_effects"]
    assert kw["prior_family"] == ("normal", "normal")
    for p in e["points"][:4]:   # (the fifth is the clamp regime, the fixtures' one documented deviation: test_reference_logjoint.py)
        th = RL.flat_theta(e, p["unconstrained"])
        c = R.cop_cells(X, W, Y[0], kw["session_duration"], th, fp_mode=kw["fp_mode"], site_re=site, obs_re=obs)
        lp = R.log_prior(th, N, T, J, Ks, Ko, kw["fp_mode"], site, obs, kw["prior_beta"], kw["prior_alpha"], kw.get("prior_fp_rate", 1.0),
                         (kw.get("prior_site_re_sd", 1.0), kw.get("prior_obs_re_sd", 1.0)))
        want = -p["U"] - lp
        assert abs(c["l"].sum() - want) <= 1e-10 * abs(want), (case, p["label"], c["l"].sum(), want)
        assert c["l"].shape == (T, N) and c["true_mean"].shape == (J, T, N)


def _data(rng, N=40, T=2, J=4):
    X, W, Y, Dur = R.make_data(rng, N, T, J, 2, 2)
    W[9, 1, :, 1] = np.nan            # a visit covariate masks its visits: period 1 of site 9 is empty
    return X, W, Y, Dur


def test_structure_of_the_cells():
    rng = np.random.default_rng(0)
    X, W, Y, Dur = _data(rng)
    th = rng.uniform(-1.0, 1.0, size=6)
    c = R.cop_cells(X, W, Y, Dur, th)
    empty = c["n_obs"] == 0
    assert empty[:, 0].all() and empty[:, 5].all() and empty[1, 9] and not empty.all()
    assert np.all(c["l"][empty] == 0.0) and np.max(np.abs(c["q"][empty] - c["psi"][empty])) <= 1e-15
    pos = c["y_sum"] > 0
    assert pos.sum() > 10 and (~pos & ~empty).sum() > 5
    assert np.all(c["q"][pos] == 1.0) and np.all(c["l"][pos] == c["A"][pos]) and np.all(np.isneginf(c["B"][pos]))   # Poisson(0) met a count
    assert np.all(c["q"][~pos & ~empty] < c["psi"][~pos & ~empty])            # zero counts only: less likely occupied than a priori
    masked = ~c["m"]
    assert masked.any() and (masked & ~empty[None]).any()
    assert np.all(c["rho"] == 1.0) and np.array_equal(c["true_mean"], c["q"][None] * c["y"])   # no rate: every counted detection is real
    bl, bq, bt = R.bounds(c, 2e-6)
    assert all(np.all(np.isfinite(b)) for b in (bl, bq, bt)) and np.all(bl > 0) and np.all(bt[masked] == 0.0)
    for mode in ("constant", "unoccupied"):
        cf = R.cop_cells(X, W, Y, Dur, np.r_[th, -1.0], fp_mode=mode)
        assert np.all(np.isfinite(cf["B"])) and (cf["q"][pos] < 1.0 - 1e-6).any() and np.all(cf["l"][empty] == 0.0)   # with a rate a count no longer proves occupancy
        assert np.all(cf["true_mean"][masked] == 0.0) and np.all(cf["y"][masked] == 0.0)
        assert np.all(cf["true_mean"].sum(0) <= cf["q"] * cf["y_sum"] * (1 + 1e-15))
        if mode == "unoccupied":
            assert np.all(cf["rho"] == 1.0)
        else:
            unm = cf["m"]
            assert np.all((cf["rho"][unm] > 0) & (cf["rho"][unm] < 1)) and np.all(cf["true_mean"][unm & (cf["y"] > 0)] < (cf["q"][None] * cf["y"])[unm & (cf["y"] > 0)])
    # random effects enter through their offsets: zero effects change nothing, one effect moves its site alone
    o = R.L.occu_theta_layout(40, 2, 4, 2, 2, True, True, True)
    thr = np.r_[th, -1.0, 0.3, -0.2, np.zeros(o["D"] - 9)]
    base = R.cop_cells(X, W, Y, Dur, np.r_[th, -1.0], fp_mode="constant")
    cr = R.cop_cells(X, W, Y, Dur, thr, fp_mode="constant", site_re=True, obs_re=True)
    assert np.allclose(cr["l"], base["l"], rtol=0, atol=1e-12)
    thr[o["u"] + 11] = 2.0
    cr = R.cop_cells(X, W, Y, Dur, thr, fp_mode="constant", site_re=True, obs_re=True)
    assert np.all(cr["psi"][:, 11] > base["psi"][:, 11])
    assert np.allclose(np.delete(cr["l"], 11, axis=1), np.delete(base["l"], 11, axis=1), rtol=0, atol=1e-12)


def test_expected_true_detections_by_hand():
    tm = np.zeros((2, 3, 1, 2, 1), dtype=np.float32)      # (n = 2, J = 3, T = 1, N = 2, S = 1)
    tm[0, :, 0, 0, 0] = [0.5, 2.25, 0.0]
    tm[0, :, 0, 1, 0] = [12.0, 1.0, 0.5]
    tm[1, :, 0, 0, 0] = [0.125, 0.0, 0.0]
    out = expected_true_detections({"true_mean": tm})
    assert out.shape == (2, 1, 2, 1) and out.dtype == np.float64
    assert np.array_equal(out[:, 0, :, 0], [[2.75, 13.5], [0.125, 0.0]])


def test_python_refusals():
    with pytest.raises(TypeError):
        conditional_counts(lambda **kw: None, None)
    with pytest.raises(TypeError):
        conditional_counts("occu_cop", None)
    others = ("occu", "occu_comb", "occu_rn", "nmixture", "occu_dyn", "occu_cs")
    assert set(others) | {"occu_cop"} == set(SERVED_BY) and len(others) + 1 == len(SERVED_BY)
    for name in others:
        with pytest.raises(NotImplementedError, match=name + r"\b.*" + SERVED_BY[name]):
            conditional_counts(getattr(models, name), None)
    # (the sampler's eighth model, occu with false positives, is the callable ``occu`` with a flag: one refusal covers both)
    # ... and the four other functions point here
    assert SERVED_BY["occu_cop"] == "conditional_counts"
    for fn in (conditional_occupancy, conditional_abundance, conditional_dynamics, conditional_scores):
        with pytest.raises(NotImplementedError, match=r"occu_cop\b.*conditional_counts"):
            fn(models.occu_cop, None)


def test_entry_point_is_declared_and_exported():
    assert "bl_count_posterior" in _ffi.EXPORTS
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "biolith_hip.h")).read()
    assert ("int bl_count_posterior(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, float *log_lik, float *z_prob, uint8_t *z,\n"
            "                       float *true_mean, int32_t *true_count);") in header
    assert "conditional_counts" in utils.__all__ and utils.conditional_counts is conditional_counts


def test_marginal_criteria_accept_the_new_result():
    rng = np.random.default_rng(1)
    X, W, Y, Dur = _data(rng, N=12, T=2, J=3)
    ths = np.r_[0.2, -0.4, 0.3, -0.5, 0.2, 0.1, -1.2] + rng.normal(scale=0.1, size=(6, 7))
    cells = [R.cop_cells(X, W, Y, Dur, t, fp_mode="constant") for t in ths]
    ll = np.stack([c["l"] for c in cells])[..., None].astype(np.float32)          # (n, T, N, 1)
    z = (rng.uniform(size=ll.shape) < np.stack([c["q"] for c in cells])[..., None]).astype(np.int32)
    lat = LazySamples(psi=np.stack([c["psi"] for c in cells])[..., None].astype(np.float32),
                      z_prob=np.stack([c["q"] for c in cells])[..., None].astype(np.float32), z=z, log_lik=ll,
                      n_obs=cells[0]["n_obs"][..., None].astype(np.int32))
    lat.set_lazy("true_mean", lambda: np.stack([c["true_mean"] for c in cells])[..., None].astype(np.float32))
    lat.set_lazy("true_count", lambda: np.zeros((6, 3, 2, 12, 1), dtype=np.int32))
    w = waic_marginal(lat)
    assert set(w) == {"waic", "p_waic", "lppd"} and all(np.isfinite(v) for v in w.values()) and w["p_waic"] > 0
    keep = cells[0]["n_obs"] > 0
    l64 = ll[..., 0].astype(np.float64)[:, keep]
    mx = l64.max(0)
    lppd = float(np.sum(mx + np.log(np.mean(np.exp(l64 - mx), axis=0))))
    assert abs(w["lppd"] - lppd) <= 1e-10 * abs(lppd) and abs(lppd_marginal(lat) - lppd) <= 1e-10 * abs(lppd)
    assert finite_sample_occupancy(lat).shape == (6, 2, 1)
    etd = expected_true_detections(lat)
    assert etd.shape == (6, 2, 12, 1) and np.all(etd[..., 0] <= cells[0]["y_sum"][None] * lat["z_prob"][..., 0].astype(np.float64) * (1 + 1e-6))


def test_draw_frequency_criterion_holds_for_the_restatement_alone():
    """What test_gpu_counts.py asserts of the device's draws, with NumPy's generator drawing from the restatement's probabilities: the
    4.5 belongs to the statistic, not to the device.  (400 repeats here, 4000 there: the statistic is standardised for either.)"""
    X, W, Y, Dur, th, _ = R.frequency_case()
    c = R.cop_cells(X, W, Y, Dur, th, fp_mode="constant")
    n = 400
    for seed in (0, 1, 2):
        rng = np.random.default_rng(seed)
        z = rng.random((n,) + c["q"].shape) < c["q"]
        t = rng.binomial(c["y"].astype(np.int64), c["rho"], size=(n,) + c["rho"].shape) * z[:, None]   # the joint draw: z Binomial(y_j, rho_j)
        got = R.pooled_statistics(c, z.sum(0), t.sum(0), n)
        assert got["z"][1] >= MIN_Z_CELLS and got["t"][1] >= MIN_T_VISITS, got     # the counts the device test relies on
        assert abs(got["z"][0]) <= 4.5 and abs(got["t"][0]) <= 4.5, (seed, got)
