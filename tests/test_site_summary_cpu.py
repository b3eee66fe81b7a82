"""site_summary without a GPU: the exports; the host's rank and interpolation rule against np.quantile on float64 input; the rank
budget; every refusal and argument check of the wrapper that comes before a device is touched.

Tolerance of the rule: NumPy's lerp and a + (b - a) g differ by one rounding -- |got - want| <= 2e-15 max(1, |want|)
(tests/summary_ref.py)."""
import numpy as np
import pytest

import summary_ref
from biolith_amd import _ffi, models
from biolith_amd.utils import site_summary
from biolith_amd.utils import site_summary as _exported
from biolith_amd.utils.site_summary import interpolate, quantile_ranks, site_names

PROBS = [0.0, 1.0, 1.0 / 3.0, 0.025, 0.05, 0.5, 0.95, 0.975]
DATA = dict(site_covs=np.zeros((4, 1), np.float32), obs_covs=np.zeros((4, 1, 2, 1), np.float32), obs=np.zeros((1, 4, 1, 2), np.float32))


class _NoPosterior:
    """Any use of the posterior -- the first step towards a device -- fails the test."""

    def get_samples(self):
        raise AssertionError("the posterior was read: the refusal came too late")


class _Posterior:
    def __init__(self, sites):
        self.sites = sites

    def get_samples(self):
        return self.sites


def _posterior(n=5, Ks=1, Ko=1):
    return _Posterior(dict(beta=np.zeros((n, 1, Ks + 1), np.float32), alpha=np.zeros((n, 1, Ko + 1), np.float32)))


def test_the_function_the_entry_and_the_cap_are_exported():
    from biolith_amd import utils

    assert "site_summary" in utils.__all__ and utils.site_summary is _exported and callable(site_summary)
    assert "bl_site_summary" in _ffi.EXPORTS and _ffi.SUMMARY_MAX_RANKS == 16
    assert "np.quantile(v, P, axis=0)" in site_summary.__doc__
    assert site_names("occu") == ("psi", "prob_detection") and site_names("occu_cs") == ("psi", "prob_detection")
    assert site_names("occu_rn") == site_names("nmixture") == ("abundance", "prob_detection")
    assert site_names("occu_cop") == ("psi", "rate_detection")


# ------------------------------------------------------------------------------------------ the rank and interpolation rule ----
@pytest.mark.parametrize("ties", [False, True], ids=["distinct", "ties"])
@pytest.mark.parametrize("n", [1, 2, 3, 7, 64, 65, 200])
def test_ranks_and_interpolation_against_numpy(n, ties):
    rng = np.random.default_rng(n)
    v32 = rng.random((n, 40)).astype(np.float32)
    if ties:
        v32 = v32[rng.integers(0, max(1, n // 3), n)]   # every column: about n / 3 distinct values
        v32[:, 0] = v32[0, 0]                           # one column: a single value
    lo, hi, g, ranks = quantile_ranks(PROBS, n)
    want_lo, want_hi, want_g, want_ranks = summary_ref.host_ranks(PROBS, n)
    assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi) and np.array_equal(g, want_g) and np.array_equal(ranks, want_ranks)
    assert ranks.size <= 16 and ranks.min() >= 0 and ranks.max() <= n - 1 and np.all(np.diff(ranks) > 0)
    got = interpolate(summary_ref.order_reference(v32, ranks), ranks, lo, hi, g)
    want = np.quantile(v32.astype(np.float64), PROBS, axis=0)
    assert got.dtype == np.float64 and got.shape == want.shape
    err = np.abs(got - want)
    print(f"n {n} ties {ties}: max |err| {err.max():.2e}")
    assert np.all(err <= 2e-15 * np.maximum(1.0, np.abs(want)))
    assert got.tobytes() == summary_ref.host_quantiles(v32, PROBS).tobytes()
    # the ends are order statistics themselves
    assert np.array_equal(got[0], v32.min(0).astype(np.float64)) and np.array_equal(got[1], v32.max(0).astype(np.float64))


def test_the_rank_budget():
    eight = np.linspace(0.05, 0.95, 8)                       # 8 distinct probs of 1000 draws: 16 ranks
    assert quantile_ranks(eight, 1000)[3].size == 16
    nine = np.append(eight, 1.0)                             # the largest value is one more rank: 17
    assert summary_ref.host_ranks(nine, 1000)[3].size == 17
    with pytest.raises(ValueError, match="at most 16"):
        quantile_ranks(nine, 1000)
    assert quantile_ranks(nine, 5)[3].size <= 5              # few draws: the ranks coincide, any number of probs passes
    with pytest.raises(ValueError, match="at most 16"):
        site_summary(models.occu, _posterior(n=1000), **DATA, probs=nine)


# ------------------------------------------------------------------------------------------ refusals before any device call ----
@pytest.mark.parametrize("name", ["occu_comb", "occu_dyn"])
def test_models_whose_sites_are_formed_on_the_host_are_refused(name):
    with pytest.raises(NotImplementedError, match=rf"site_summary\(\): not built for {name} .*predict\(\) followed by np.mean"):
        site_summary(getattr(models, name), _NoPosterior(), **DATA)


def test_not_a_model_is_a_type_error():
    with pytest.raises(TypeError, match="biolith_amd model"):
        site_summary(lambda **kw: None, _NoPosterior(), **DATA)
    with pytest.raises(TypeError, match="biolith_amd model"):
        site_summary("occu", _NoPosterior(), **DATA)


@pytest.mark.parametrize("probs,message", [((), "empty"), ((0.5, 1.5), r"\[0, 1\]"), ((-0.1,), r"\[0, 1\]"), ((np.nan,), r"\[0, 1\]")])
def test_bad_probs_are_value_errors(probs, message):
    with pytest.raises(ValueError, match=message):
        site_summary(models.occu, _NoPosterior(), **DATA, probs=probs)


@pytest.mark.parametrize("model,sites", [("occu", ("abundance",)), ("occu_rn", ("psi",)), ("occu_cop", ("prob_detection",)), ("occu", ()),
                                         ("occu", ("psi", "z"))])
def test_unknown_sites_are_value_errors(model, sites):
    with pytest.raises(ValueError, match="`sites` must name some of"):
        site_summary(getattr(models, model), _NoPosterior(), **DATA, sites=sites)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_posterior_sites_are_value_errors(bad):
    posterior = _posterior()
    posterior.sites["alpha"][3, 0, 1] = bad
    with pytest.raises(ValueError, match="'alpha' holds non-finite draws"):
        site_summary(models.occu, posterior, **DATA)


def test_covariate_counts_that_differ_from_the_coefficients_are_value_errors():
    with pytest.raises(ValueError, match="covariate counts differ"):
        site_summary(models.occu, _posterior(Ks=2), **DATA)
    with pytest.raises(ValueError, match="covariate counts differ"):
        site_summary(models.occu, _posterior(Ko=3), **DATA)


def test_no_draws_is_a_value_error():
    with pytest.raises(ValueError, match="no draws"):
        site_summary(models.occu, _posterior(n=0), **DATA)
