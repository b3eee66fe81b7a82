"""conditional_scores without a device: the float64 restatement (tests/scores_ref.py) against brute-force enumeration of z and all
2^J values of f, the Python refusals, the declarations of the entry, expected_true_positives by hand, and the marginal criteria on a
synthetic result with the new keys."""
import os

import numpy as np
import pytest

import scores_ref as R
from biolith_amd import _ffi, models, utils
from biolith_amd.evaluation import expected_true_positives, finite_sample_occupancy, lppd_marginal, waic_marginal
from biolith_amd.utils import conditional_abundance, conditional_dynamics, conditional_occupancy, conditional_scores
from biolith_amd.utils._conditional import SERVED_BY
from biolith_amd.utils.mcmc import LazySamples


def _tiny_case():
    """N = 4, T = 2, J = 3, one covariate a side; a missing score, a missing visit covariate, a fully masked cell, a site without
    its covariate (both its cells masked)."""
    rng = np.random.default_rng(5)
    N, T, J = 4, 2, 3
    X, W = rng.normal(size=(N, 1)), rng.normal(size=(N, T, J, 1))
    Sc = rng.normal(loc=4.0, scale=6.0, size=(N, T, J))
    Sc[0, 0, 1] = np.nan          # one masked visit
    W[1, 1, 2, 0] = np.nan        # one masked through its covariate
    Sc[2, 1, :] = np.nan          # a fully masked cell
    X[3, 0] = np.nan              # a site whose visits are all masked
    th = np.array([0.3, -0.8, -0.4, 0.9, 0.5, np.log(9.0), np.log(7.0), np.log(4.0)])
    X, W, Sc = (a.astype(np.float32).astype(np.float64) for a in (X, W, Sc))   # what the engine holds
    return X, W, Sc, th


def test_restatement_matches_brute_force_enumeration():
    X, W, Sc, th = _tiny_case()
    c = R.cs_cells(X, W, Sc, th)
    beta, alpha, mu0, mu1, sg0, sg1 = R.split(th, 1, 1)
    N, T, J = Sc.shape
    assert c["l"].shape == (T, N) and c["f_prob"].shape == (J, T, N)
    Xz, Wz = np.nan_to_num(X), np.nan_to_num(W)
    masked_visits = 0
    for i in range(N):
        psi = 1 / (1 + np.exp(-(beta[0] + Xz[i] @ beta[1:])))
        for t in range(T):
            p = 1 / (1 + np.exp(-(alpha[0] + Wz[i, t] @ alpha[1:])))
            m = np.isfinite(Sc[i, t]) & ~np.isnan(W[i, t]).any(-1) & ~np.isnan(X[i]).any()
            ll, qz, qf = R.brute_force_cell(psi, p, m, np.nan_to_num(Sc[i, t]), mu0, mu1, sg0, sg1)
            assert c["n_obs"][t, i] == m.sum()
            assert abs(c["l"][t, i] - ll) <= 1e-12 * max(1.0, abs(ll)), (i, t)
            assert abs(c["q"][t, i] - qz) <= 1e-12 and np.all(np.abs(c["f_prob"][:, t, i] - qf) <= 1e-12), (i, t)
            assert np.array_equal(c["m"][:, t, i], m)
            for j in np.flatnonzero(~m):   # no score to condition on: f_prob = z_prob p_j
                assert abs(c["f_prob"][j, t, i] - c["q"][t, i] * p[j]) <= 1e-15 and abs(c["r"][j, t, i] - p[j]) <= 1e-15
                masked_visits += 1
            if not m.any():                # nothing observed: the prior
                assert c["l"][t, i] == 0.0 and abs(c["q"][t, i] - psi) <= 1e-15
    assert masked_visits == 2 + 3 + 6 and (c["n_obs"] == 0).sum() == 3
    bl, bq, bf = R.bounds(c, 2e-6)
    assert bl.shape == bq.shape == (T, N) and bf.shape == (J, T, N) and np.all(bf >= bq[None]) and np.all(bl > 0)


def test_python_refusals():
    with pytest.raises(TypeError):
        conditional_scores(lambda **kw: None, None)
    with pytest.raises(TypeError):
        conditional_scores("occu_cs", None)
    for name in ("occu", "occu_comb", "occu_rn", "nmixture", "occu_dyn"):
        with pytest.raises(NotImplementedError, match=name + r"\b.*" + SERVED_BY[name]):
            conditional_scores(getattr(models, name), None)
    with pytest.raises(NotImplementedError, match=r"occu_cop\b"):
        conditional_scores(models.occu_cop, None)
    # ... and the three other functions point here
    assert SERVED_BY["occu_cs"] == "conditional_scores"
    for fn in (conditional_occupancy, conditional_abundance, conditional_dynamics):
        with pytest.raises(NotImplementedError, match=r"occu_cs\b.*conditional_scores"):
            fn(models.occu_cs, None)


def test_entry_point_is_declared_and_exported():
    assert "bl_score_posterior" in _ffi.EXPORTS
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "biolith_hip.h")).read()
    assert ("int bl_score_posterior(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, float *log_lik, float *z_prob, uint8_t *z,\n"
            "                       float *f_prob, uint8_t *f);") in header
    assert "#define BL_ABI_VERSION 1" in header
    assert "conditional_scores" in utils.__all__ and utils.conditional_scores is conditional_scores


def test_expected_true_positives_by_hand():
    f_prob = np.zeros((2, 3, 1, 2, 1), dtype=np.float32)      # (n = 2, J = 3, T = 1, N = 2, S = 1)
    f_prob[0, :, 0, 0, 0] = [0.5, 0.25, 0.0]
    f_prob[0, :, 0, 1, 0] = [1.0, 1.0, 0.5]
    f_prob[1, :, 0, 0, 0] = [0.125, 0.0, 0.0]
    out = expected_true_positives({"f_prob": f_prob})
    assert out.shape == (2, 1, 2, 1) and out.dtype == np.float64
    assert np.array_equal(out[:, 0, :, 0], [[0.75, 2.5], [0.125, 0.0]])


def test_marginal_criteria_accept_the_new_result():
    X, W, Sc, th = _tiny_case()
    rng = np.random.default_rng(1)
    ths = th + rng.normal(scale=0.1, size=(6, th.size))
    cells = [R.cs_cells(X, W, Sc, t) for t in ths]
    ll = np.stack([c["l"] for c in cells])[..., None].astype(np.float32)          # (n, T, N, 1)
    z = (rng.uniform(size=ll.shape) < np.stack([c["q"] for c in cells])[..., None]).astype(np.int32)
    lat = LazySamples(psi=np.stack([c["psi"] for c in cells])[..., None].astype(np.float32),
                      z_prob=np.stack([c["q"] for c in cells])[..., None].astype(np.float32), z=z, log_lik=ll,
                      n_obs=cells[0]["n_obs"][..., None].astype(np.int32))
    lat.set_lazy("f_prob", lambda: np.stack([c["f_prob"] for c in cells])[..., None].astype(np.float32))
    lat.set_lazy("f", lambda: np.zeros((6, 3, 2, 4, 1), dtype=np.int32))
    w = waic_marginal(lat)
    assert set(w) == {"waic", "p_waic", "lppd"} and all(np.isfinite(v) for v in w.values()) and w["p_waic"] > 0
    keep = cells[0]["n_obs"] > 0
    l64 = ll[..., 0].astype(np.float64)[:, keep]
    lppd = float(np.sum(np.log(np.mean(np.exp(l64), axis=0))))
    assert abs(w["lppd"] - lppd) <= 1e-10 * abs(lppd) and abs(lppd_marginal(lat) - lppd) <= 1e-10 * abs(lppd)
    assert finite_sample_occupancy(lat).shape == (6, 2, 1)
    etp = expected_true_positives(lat)
    assert etp.shape == (6, 2, 4, 1) and np.all(etp <= 3.0 * lat["z_prob"].astype(np.float64) + 1e-6)


def test_draw_frequency_criterion_holds_for_the_restatement_alone():
    """What test_gpu_scores.py asserts of the device's draws, with NumPy's generator drawing from the restatement's probabilities: the
    4.5 belongs to the statistic, not to the device.  (400 repeats here, 4000 there: the statistic is standardised for either.)"""
    X, W, Sc, th, _ = R.frequency_case()
    c = R.cs_cells(X, W, Sc, th)
    n = 400
    for seed in (0, 1, 2):
        rng = np.random.default_rng(seed)
        z = rng.random((n,) + c["q"].shape) < c["q"]
        f = (rng.random((n,) + c["r"].shape) < c["r"]) & z[:, None]           # the joint draw: f_j = z Bernoulli(r_j)
        got = R.pooled_statistics(c, z.sum(0), f.sum(0), n)
        assert got["z"][1] >= 1000 and got["f"][1] >= 8000, got                # the counts the device test relies on
        assert abs(got["z"][0]) <= 4.5 and abs(got["f"][0]) <= 4.5, (seed, got)
