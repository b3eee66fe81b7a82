"""occu_comb's predictive evaluation without a GPU: ``log_likelihood_comb`` against the reference-pinned float64 restatement
(tests/comb_ref.py, itself held to the reference model's own log-joint), its masks, ``waic_comb`` against a direct evaluation, and the
refusals around ``predict_comb``.  Host only: the "posteriors" are made by hand, nothing is fitted."""
import contextlib
import io
import math

import numpy as np
import pytest
from scipy.special import logsumexp

from biolith_amd.evaluation import log_likelihood_comb, waic_comb
from biolith_amd.models import occu, occu_comb, simulate_comb
from biolith_amd.utils import predict_comb
from comb_ref import from_data, reference_case


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _sites(ref, thetas, z):
    """predict_comb's sites for the draws ``thetas`` (n, D) of one species, made in float64 NumPy and cast to float32; ``z`` (n, T, N)."""
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    pc, aru, ex = [], [], []
    for th in np.atleast_2d(thetas):
        _, apc, aar, e = ref.split(np.asarray(th, dtype=np.float64))
        pc.append(_sigmoid(apc[0] + ref.Wp @ apc[1:]).transpose(2, 1, 0))   # (Jpc, T, N)
        aru.append(_sigmoid(aar[0] + ref.Wa @ aar[1:]).transpose(2, 1, 0))
        ex.append([_sigmoid(e[0]), _sigmoid(e[1]), e[2], e[2] + math.exp(e[3]), math.exp(e[4]), math.exp(e[5])])
    ex = np.asarray(ex)
    ps = {"z": np.asarray(z, dtype=np.int32)[..., None], "PC_prob_detection": f32(pc)[..., None], "ARU_prob_detection": f32(aru)[..., None]}
    for c, k in enumerate(("ARU_prob_fp_constant", "ARU_fp_unoccupied", "mu0", "mu1", "sigma0", "sigma1")):
        ps[k] = f32(ex[:, c:c + 1])
    return ps


@pytest.mark.parametrize("case", ["comb_missing_3periods", "comb_missing", "comb_clamp"])
def test_log_likelihood_comb_sums_to_the_reference_pinned_likelihood(case):
    """Per site-period logaddexp(log psi + sum ll[z = 1], log(1 - psi) + sum ll[z = 0]), summed over everything, is CombRef.log_lik(theta):
    the masks, the clamp (a point-count detection at z = 0 costs log tiny) and all three blocks at once.  Bound: relative 1e-5, the
    one tests/test_gpu_comb.py holds the comb potential to.  Achieved with float32 sites evaluated in float64: at most 9.9e-9 over the
    cases and points below (printed)."""
    data, pri, fx = reference_case(case)
    ref = from_data(data, **pri)
    N, T = ref.Yp.shape[:2]
    d = {k: data[k] for k in ("site_covs", "PC_obs_covs", "ARU_obs_covs", "PC_obs", "ARU_obs", "scores_obs")}
    for pt in fx["points"]:
        th = np.asarray(pt["theta"], dtype=np.float64)
        beta = ref.split(th)[0]
        psi = _sigmoid(beta[0] + ref.X @ beta[1:])[None, :]                                  # (1, N)
        cell = []
        for z in (1, 0):
            ll = log_likelihood_comb(_sites(ref, th, np.full((1, T, N), z)), **d, coords=None, ell=0.0)
            assert {k: v.shape for k, v in ll.items()} == {"y_pc": (1, ref.Yp.shape[2], T, N, 1), "y_aru": (1, ref.Ya.shape[2], T, N, 1),
                                                           "scores": (1, ref.Sc.shape[2], T, N, 1)}
            cell.append(sum(v.astype(np.float64)[0, ..., 0].sum(axis=0) for v in ll.values()))   # (T, N)
        total = np.logaddexp(np.log(psi) + cell[0], np.log1p(-psi) + cell[1]).sum()
        want = ref.log_lik(th)
        print(f"{case}: log_lik {want:.6f}, from log_likelihood_comb {total:.6f}, relative {abs(total - want) / abs(want):.2e}")
        assert abs(total - want) <= 1e-5 * abs(want), (total, want)


def test_a_point_count_detection_at_z0_costs_log_tiny():
    data, pri, fx = reference_case("comb_clamp")
    ref = from_data(data, **pri)
    N, T = ref.Yp.shape[:2]
    ll = log_likelihood_comb(_sites(ref, fx["points"][0]["theta"], np.zeros((1, T, N))), **data)["y_pc"][0, ..., 0]
    det = (ref.mp & (ref.Yp > 0)).transpose(2, 1, 0)
    assert det.any() and np.all(ll[det] == np.float32(math.log(np.finfo(np.float32).tiny)))
    assert np.all(ll[~det] > -1e-30)   # a non-detection at z = 0 costs log1p(-tiny) = 0; a masked visit 0


def _plain(n_sites=12, seed=4):
    with contextlib.redirect_stdout(io.StringIO()):
        data, _ = simulate_comb(n_sites=n_sites, n_periods=2, PC_replicates=3, ARU_replicates=5, scores_replicates=4,
                                ARU_prob_fp_constant=0.05, ARU_prob_fp_unoccupied=0.1, random_seed=seed)
    th = np.linspace(-0.5, 0.5, 12)
    th[-6:] = [-1.0, -1.2, -2.0, math.log(4.0), math.log(5.0), math.log(3.0)]
    return data, th


def test_log_likelihood_comb_masks():
    data, th = _plain()
    z = np.random.default_rng(0).integers(0, 2, size=(1, 2, 12))
    base = log_likelihood_comb(_sites(from_data(data), th, z), **data)
    assert all(np.all(v != 0) for v in base.values())
    # a NaN ARU covariate zeroes that visit only (the sites are the model's: the covariate reads as 0)
    d2 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in data.items()}
    d2["ARU_obs_covs"][3, 1, 2, 0] = np.nan
    ll = log_likelihood_comb(_sites(from_data(d2), th, z), **d2)
    hit = np.zeros(base["y_aru"].shape, dtype=bool)
    hit[0, 2, 1, 3, 0] = True
    assert ll["y_aru"][hit] == 0 and np.array_equal(ll["y_aru"][~hit], base["y_aru"][~hit])
    assert np.array_equal(ll["y_pc"], base["y_pc"]) and np.array_equal(ll["scores"], base["scores"])
    # a NaN point-count covariate: that point count only
    d2 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in data.items()}
    d2["PC_obs_covs"][5, 0, 1, 0] = np.nan
    ll = log_likelihood_comb(_sites(from_data(d2), th, z), **d2)
    assert ll["y_pc"][0, 1, 0, 5, 0] == 0 and np.count_nonzero(ll["y_pc"] == 0) == 1
    assert np.array_equal(ll["y_aru"], base["y_aru"]) and np.array_equal(ll["scores"], base["scores"])
    # a NaN score: itself only
    d2 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in data.items()}
    d2["scores_obs"][0, 7, 1, 3] = np.nan
    ll = log_likelihood_comb(_sites(from_data(d2), th, z), **d2)
    assert ll["scores"][0, 3, 1, 7, 0] == 0 and np.count_nonzero(ll["scores"] == 0) == 1
    # a NaN site covariate zeroes every entry of the site in all three blocks, and nothing else
    d3 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in data.items()}
    d3["site_covs"][1, 0] = np.nan
    ll = log_likelihood_comb(_sites(from_data(d3), th, z), **d3)
    for k, v in ll.items():
        assert np.all(v[:, :, :, 1] == 0), k
        others = np.delete(v, 1, axis=3)
        assert np.all(others != 0) and np.array_equal(others, np.delete(base[k], 1, axis=3)), k


def test_waic_comb_against_a_direct_evaluation():
    with contextlib.redirect_stdout(io.StringIO()):
        data, _ = simulate_comb(n_sites=12, n_periods=2, PC_replicates=3, ARU_replicates=5, scores_replicates=4, ARU_prob_fp_constant=0.05,
                                ARU_prob_fp_unoccupied=0.1, simulate_missing=True, random_seed=6)
    _, th = _plain()
    rng = np.random.default_rng(1)
    thetas = th[None] + rng.normal(0, 0.2, size=(3, 12))
    # z = 1 wherever a point count was made (a detection at z = 0 would cost log tiny in every draw alike), random elsewhere
    seen = (np.nan_to_num(data["PC_obs"][0]).sum(-1) > 0).T[None]
    z = np.where(seen, 1, rng.integers(0, 2, size=(3, 2, 12)))
    ps = _sites(from_data(data), thetas, z)
    ll = log_likelihood_comb(ps, **data)
    ref = from_data(data)
    cols = []
    for key, mask in (("y_pc", ref.mp), ("y_aru", ref.ma), ("scores", ref.ms)):   # (N, T, J) masks, written independently in comb_ref
        for i, t, j in zip(*np.nonzero(mask)):
            cols.append(ll[key][:, j, t, i, 0].astype(np.float64))
    cols = np.asarray(cols).T                                                       # (3, points)
    assert cols.shape[1] == ref.mp.sum() + ref.ma.sum() + ref.ms.sum() and cols.shape[1] < ref.mp.size + ref.ma.size + ref.ms.size
    lppd = float(np.sum(logsumexp(cols, axis=0) - math.log(3)))
    p_waic = float(np.sum(np.var(cols, axis=0, ddof=1)))
    w = waic_comb(ps, **data)
    assert set(w) == {"waic", "p_waic", "lppd"}
    assert w["lppd"] == pytest.approx(lppd, rel=1e-12) and w["p_waic"] == pytest.approx(p_waic, rel=1e-12)
    assert w["waic"] == pytest.approx(-2 * (lppd - p_waic), rel=1e-12) and w["p_waic"] > 0 and math.isfinite(w["waic"])


def test_predict_comb_refuses_other_models():
    data, _ = _plain()
    with pytest.raises(NotImplementedError, match="occu "):
        predict_comb(occu, None, **{k: data[k] for k in ("site_covs", "PC_obs_covs", "ARU_obs_covs", "scores_obs")})
    with pytest.raises(TypeError):
        predict_comb(lambda **kw: None, None, data["site_covs"], data["PC_obs_covs"], data["ARU_obs_covs"], data["scores_obs"])
