"""PSIS-LOO without a GPU: the float64 restatement (tests/psis_ref.py) is anchored to what it must estimate -- an exact leave-one-out
density and the shape of an exact Pareto tail -- and to the definition's edge cases; ``compare_marginal`` and ``loo_marginal``'s checks
are host arithmetic.  The device kernels are compared with the same restatement in tests/test_gpu_loo.py."""
import os
import re

import numpy as np
import pytest

import psis_ref
from biolith_amd import _ffi, utils
from biolith_amd.utils import compare_marginal, loo_marginal
from biolith_amd.utils import loo as loo_module
from conftest import ROOT


def test_exact_leave_one_out_of_a_normal_mean():
    """y_i ~ N(mu, 1) with a flat prior: mu | y ~ N(mean y, 1/30) and p(y_i | y_-i) = N(mean y_-i, 1 + 1/29) in closed form.  The bounds
    (0.03 per point, 0.05 in the sum) are several times what 4000 draws gave over five seeds (at most 0.0081 and 0.0121, largest k
    0.24); y_0 = 3.5 is the outlier whose ratios have the heaviest tail."""
    rng = np.random.default_rng(0)
    y = rng.normal(0.0, 1.0, 30)
    y[0] = 3.5
    mu = rng.normal(y.mean(), 1.0 / np.sqrt(30.0), 4000)
    ll = (-0.5 * np.log(2 * np.pi) - 0.5 * (y[None, :] - mu[:, None]) ** 2).astype(np.float32)
    elpd, k, lppd = psis_ref.matrix(ll)
    loo_mean = (y.sum() - y) / 29.0
    var = 1.0 + 1.0 / 29.0
    exact = -0.5 * np.log(2 * np.pi * var) - 0.5 * (y - loo_mean) ** 2 / var
    print("exact LOO: max |elpd_i - exact| %.4f, |sum| %.4f, max k %.3f" % (np.abs(elpd - exact).max(), abs(elpd.sum() - exact.sum()), k.max()))
    assert np.abs(elpd - exact).max() < 0.03
    assert abs(elpd.sum() - exact.sum()) < 0.05
    assert np.all(k < 0.5) and np.argmax(k) == 0
    assert np.all(elpd < lppd)   # leaving a point out never helps predicting it


@pytest.mark.parametrize("k0", [0.2, 0.5, 0.7, 1.0])
def test_k_hat_recovers_the_shape_of_an_exact_pareto_tail(k0):
    """Ratios (1 - u)^(-k0) are exactly generalised-Pareto above any cutoff: the mean k-hat of 20 columns of 4000 is within 0.1 of k0
    (the prior of weight 10 at 0.5 pulls a 190-draw tail by at most 0.05 (k0 - 0.5) / 1)."""
    rng = np.random.default_rng(0)
    u = rng.uniform(size=(4000, 20))
    ll = (k0 * np.log1p(-u)).astype(np.float32)   # ll = -log ratio
    k = psis_ref.matrix(ll)[1]
    print("k0 %.1f: mean k-hat %.3f" % (k0, k.mean()))
    assert np.all(np.isfinite(k)) and abs(k.mean() - k0) < 0.1


def test_constant_column():
    for c, n in ((-2.5, 100), (-80.0, 4000), (0.0, 7)):
        elpd, k, lppd = psis_ref.column(np.full(n, c, dtype=np.float32))
        assert k == np.inf
        assert abs(elpd - c) < 1e-12 and abs(lppd - c) < 1e-12   # (log n is added and subtracted: equal to rounding)


def test_short_tails_are_not_smoothed():
    """M = ceil(min(n / 5, 3 sqrt(n))): 16 and 20 draws give 4, which is no tail to fit; 25 give 5."""
    rng = np.random.default_rng(1)
    assert [psis_ref.tail_length(n) for n in (2, 4, 16, 20, 25, 4000, 8192)] == [1, 1, 4, 4, 5, 190, 272]
    for n in (2, 4, 16, 20):
        elpd, k, lppd = psis_ref.column(rng.normal(-3, 0.5, n).astype(np.float32))
        assert k == np.inf and np.isfinite(elpd) and elpd < lppd
    elpd, k, lppd = psis_ref.column(rng.normal(-3, 0.5, 25).astype(np.float32))
    assert np.isfinite(k) and np.isfinite(elpd) and elpd < lppd
    # without smoothing the estimate is the harmonic mean of the likelihoods
    ll = rng.normal(-3, 0.5, 16).astype(np.float32).astype(np.float64)
    assert abs(psis_ref.column(ll)[0] - (np.log(16.0) - np.log(np.sum(np.exp(-ll))))) < 1e-12


def test_a_column_of_mostly_tied_values_has_a_finite_k():
    """3000 of 4000 draws share one log-likelihood (the largest, so the ties are the smallest ratios and the tail is made of the rest)."""
    rng = np.random.default_rng(2)
    ll = rng.normal(-3, 0.3, 4000).astype(np.float32)
    ll[rng.permutation(4000)[:3000]] = np.float32(-1.5)
    elpd, k, lppd = psis_ref.column(ll)
    assert np.isfinite(k) and np.isfinite(elpd) and elpd < lppd
    # ties need no rule: any order of the draws gives the same k and, to rounding, the same elpd
    e2, k2, _ = psis_ref.column(ll[::-1])
    assert k2 == k and abs(e2 - elpd) < 1e-12


def _pointwise(elpd_i, p_loo=1.0):
    elpd_i = np.asarray(elpd_i, dtype=np.float64)
    return {"elpd_loo": float(np.nansum(elpd_i)), "p_loo": p_loo, "elpd_loo_i": elpd_i}


def test_compare_marginal():
    rng = np.random.default_rng(3)
    a = rng.normal(-2, 0.5, (3, 40))
    a[1, 5] = a[2, 7] = np.nan
    b, c = a - np.abs(rng.normal(0.1, 0.05, a.shape)), a - np.abs(rng.normal(0.3, 0.2, a.shape))
    rows = compare_marginal({"b": _pointwise(b, 2.0), "a": _pointwise(a, 3.0), "c": _pointwise(c, 4.0)})
    assert [r["name"] for r in rows] == ["a", "b", "c"]
    assert [r["p_loo"] for r in rows] == [3.0, 2.0, 4.0]
    assert rows[0]["elpd_diff"] == 0.0 and rows[0]["se_diff"] == 0.0
    ok = ~np.isnan(a)
    for r, other in zip(rows[1:], (b, c)):
        d = (other - a)[ok]
        assert r["elpd_diff"] == pytest.approx(d.sum(), rel=1e-12) and r["elpd_diff"] < 0
        assert r["se_diff"] == pytest.approx(np.sqrt(ok.sum() * np.var(d)), rel=1e-12) and r["se_diff"] > 0
        assert r["elpd_loo"] == pytest.approx(np.nansum(other), rel=1e-12)
    shifted = b.copy()
    shifted[1, 5], shifted[1, 6] = shifted[1, 6], np.nan
    with pytest.raises(ValueError, match="different cells"):
        compare_marginal({"a": _pointwise(a), "b": _pointwise(shifted)})
    with pytest.raises(ValueError, match="pointwise=True"):
        compare_marginal({"a": {"elpd_loo": 0.0, "p_loo": 0.0}})
    assert compare_marginal({}) == []


def test_loo_marginal_refuses_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device entry was reached")

    monkeypatch.setattr(loo_module, "psis_loo", no_device)
    n_obs = np.array([[2, 0, 1], [3, 3, 0]])
    good = np.random.default_rng(4).normal(-3, 0.3, (10, 2, 3)).astype(np.float32)
    with pytest.raises(ValueError, match="do not belong together"):
        loo_marginal({"log_lik": good[:, :1], "n_obs": n_obs})
    with pytest.raises(ValueError, match="1 draw"):
        loo_marginal({"log_lik": good[:1], "n_obs": n_obs})
    big = np.zeros((_ffi.PSIS_MAX_DRAWS + 1, 2, 3), dtype=np.float32)
    with pytest.raises(ValueError, match=str(_ffi.PSIS_MAX_DRAWS)):
        loo_marginal({"log_lik": big, "n_obs": n_obs})
    for bad in (np.nan, -np.inf, np.inf):
        ll = good.copy()
        ll[3, 1, 0] = bad
        with pytest.raises(ValueError, match="not finite in 1 of the 4 cells"):
            loo_marginal({"log_lik": ll, "n_obs": n_obs})
    ll = good.copy()
    ll[3, 0, 1] = np.nan   # a cell without data may hold anything: the check passes and the device entry is the next thing called
    with pytest.raises(AssertionError, match="device entry"):
        loo_marginal({"log_lik": ll, "n_obs": n_obs})


def test_loo_marginal_host_arithmetic(monkeypatch):
    """With the restatement in the device entry's place: the cells with data only, the sums, the standard error, the k counts and the
    pointwise arrays."""
    seen = {}

    def stand_in(cols, device=0, cells_per_launch=0):
        seen["shape"], seen["dtype"] = cols.shape, cols.dtype
        return psis_ref.matrix(cols)

    monkeypatch.setattr(loo_module, "psis_loo", stand_in)
    rng = np.random.default_rng(5)
    ll = rng.normal(-3, 0.4, (200, 2, 6)).astype(np.float32)
    ll[:, 1, 2] = -np.log1p(-rng.uniform(size=200)).astype(np.float32) * -1.2   # a heavy tail: k-hat far above 0.7
    n_obs = np.array([[1, 2, 0, 3, 1, 1], [2, 2, 4, 0, 0, 1]])
    ll[:, 0, 2] = 0.0
    out = loo_marginal({"log_lik": ll, "n_obs": n_obs}, pointwise=True)
    assert seen == {"shape": (200, 9), "dtype": np.float32}
    e, k, l = psis_ref.matrix(ll[:, n_obs > 0])
    assert out["n_cells"] == 9 and out["n_draws"] == 200
    assert out["elpd_loo"] == pytest.approx(e.sum(), rel=1e-14) and out["lppd"] == pytest.approx(l.sum(), rel=1e-14)
    assert out["p_loo"] == pytest.approx(l.sum() - e.sum(), rel=1e-12) and out["p_loo"] > 0
    assert out["looic"] == -2 * out["elpd_loo"]
    assert out["se"] == pytest.approx(np.sqrt(9 * np.var(e)), rel=1e-14)
    assert out["pareto_k_max"] == k.max() and out["n_k_above_0.7"] == int((k > 0.7).sum()) >= 1
    assert out["elpd_loo_i"].shape == n_obs.shape and np.array_equal(np.isnan(out["elpd_loo_i"]), n_obs == 0)
    assert np.array_equal(out["elpd_loo_i"][n_obs > 0], e) and np.array_equal(out["pareto_k"][n_obs > 0], k)
    assert "elpd_loo_i" not in loo_marginal({"log_lik": ll, "n_obs": n_obs})
    # inf counts as above 0.7
    short = loo_marginal({"log_lik": ll[:10], "n_obs": n_obs})
    assert short["pareto_k_max"] == np.inf and short["n_k_above_0.7"] == 9


def test_exports_and_constants():
    assert "bl_psis_loo" in _ffi.EXPORTS
    assert "loo_marginal" in utils.__all__ and "compare_marginal" in utils.__all__
    assert utils.loo_marginal is loo_marginal and utils.compare_marginal is compare_marginal
    header = open(os.path.join(ROOT, "include", "biolith_hip.h")).read()
    assert int(re.search(r"#define BL_PSIS_MAX_DRAWS (\d+)", header).group(1)) == _ffi.PSIS_MAX_DRAWS >= 8192
    assert psis_ref.LOG_DBL_MIN == float(np.log(np.finfo(np.float64).tiny))
    src = open(os.path.join(ROOT, "biolith_amd", "csrc", "psis_loo.hip")).read()
    assert float(re.search(r"PSIS_LOG_DBL_MIN = (-[0-9.]+);", src).group(1)) == psis_ref.LOG_DBL_MIN
    tail_max = int(re.search(r"BL_PSIS_TAIL_MAX = (\d+);", open(os.path.join(ROOT, "biolith_amd", "csrc", "psis_loo.hpp")).read()).group(1))
    assert tail_max == psis_ref.tail_length(_ffi.PSIS_MAX_DRAWS)
