"""information_criteria without a GPU: the export and the docstring's contract, the refusals and the argument checks -- all of them in
front of any device call -- and a NumPy restatement of the two streaming reductions the point kernel performs (predictive_density.hip),
checked against ``scipy.special.logsumexp`` and ``np.var(ddof=1)``.  The restatement documents the algorithm the kernel must follow:
per strip of draws a running maximum with a scaled sum of exponentials and Welford's mean / M2; the strips merged in order by a
log-sum-exp merge and Chan's pairwise merge."""
import numpy as np
import pytest
from scipy.special import logsumexp

from biolith_amd import models


class _NoPosterior:
    """Any use of the posterior -- the first step towards a device -- fails the test."""

    def get_samples(self):
        raise AssertionError("the posterior was read: the refusal came too late")


class _Posterior:
    def __init__(self, sites):
        self.sites = sites

    def get_samples(self):
        return self.sites


DATA = dict(site_covs=np.zeros((4, 1), np.float32), obs_covs=np.zeros((4, 1, 2, 1), np.float32), obs=np.zeros((1, 4, 1, 2), np.float32))


def test_information_criteria_is_exported_with_its_contract():
    from biolith_amd import utils
    from biolith_amd.utils import information_criteria

    assert "information_criteria" in utils.__all__ and utils.information_criteria is information_criteria
    doc = " ".join(information_criteria.__doc__.split())
    for line in ('ic["waic"], ic["lppd"], ic["p_waic"] ~ evaluation.waic(m, preds, **data)',
                 'ic["deviance"] ~ evaluation.deviance(m, preds, **data)',
                 'form="marginal" ~ waic_manual(preds, data) / lppd_manual(preds, data) / deviance_manual(preds, data)',
                 "differs from the host path only by the host's float32 evaluation of ``log``",
                 "With a false-positive rate the host forms ``prob_detection_fp`` in float32"):
        assert line in doc, line


def test_the_entry_is_declared():
    from biolith_amd import _ffi

    assert "bl_predictive_density" in _ffi.EXPORTS


@pytest.mark.parametrize("name", ["occu_rn", "occu_cop", "nmixture", "occu_cs", "occu_comb", "occu_dyn"])
def test_other_models_are_refused_before_any_device_call(name):
    from biolith_amd.utils import information_criteria

    with pytest.raises(NotImplementedError, match=rf"information_criteria\(\): not built for {name} \(built: occu "):
        information_criteria(getattr(models, name), _NoPosterior(), **DATA)


def test_not_a_model_is_a_type_error():
    from biolith_amd.utils import information_criteria

    with pytest.raises(TypeError, match="biolith_amd model"):
        information_criteria(lambda **kw: None, _NoPosterior(), **DATA)


def test_bad_form_and_missing_obs():
    from biolith_amd.utils import information_criteria

    with pytest.raises(ValueError, match="`form` must be one of"):
        information_criteria(models.occu, _NoPosterior(), **DATA, form="joint")
    with pytest.raises(ValueError, match="obs is required"):
        information_criteria(models.occu, _NoPosterior(), site_covs=DATA["site_covs"], obs_covs=DATA["obs_covs"])


def test_wrong_shapes_and_species_count():
    from biolith_amd.utils import information_criteria

    sites = lambda S, Ks=1, Ko=1: _Posterior(dict(beta=np.zeros((3, S, Ks + 1), np.float32), alpha=np.zeros((3, S, Ko + 1), np.float32)))
    with pytest.raises(ValueError, match="obs must be of shape"):
        information_criteria(models.occu, _NoPosterior(), **{**DATA, "obs": np.zeros((1, 4, 1, 3), np.float32)})
    with pytest.raises(ValueError, match="obs must be of shape"):
        information_criteria(models.occu, _NoPosterior(), **{**DATA, "obs": np.zeros((4, 1, 2), np.float32)})
    with pytest.raises(ValueError, match="obs has 1 species, the posterior 2"):
        information_criteria(models.occu, sites(2), **DATA)
    with pytest.raises(ValueError, match="covariate counts differ"):
        information_criteria(models.occu, sites(1, Ks=2), **DATA)


# ------------------------------------------------------------------------------------------ the streaming reductions, restated ----
def strip_bounds(n, R):
    """The draws dealt to R strips in order, as evenly as they go (bl_pd_strip_begin): the first n % R strips take one more."""
    base, rem = divmod(n, R)
    begin = [r * base + min(r, rem) for r in range(R + 1)]
    return list(zip(begin[:-1], begin[1:]))


def walk_strip(ll):
    """One thread's walk over its strip: (count, running maximum m, s = sum exp(ll - m), Welford's mean, M2)."""
    m, s, mean, m2 = -np.inf, 0.0, 0.0, 0.0
    for k, x in enumerate(ll, start=1):
        if x > m:
            s = s * np.exp(m - x) + 1.0      # (the first value: 0 * exp(-inf) + 1)
            m = x
        else:
            s += np.exp(x - m)
        delta = x - mean
        mean += delta / k
        m2 += delta * (x - mean)
    return len(ll), m, s, mean, m2


def merge_strips(parts):
    """The finish kernel: the strips' partials in strip order -> (log mean exp, variance with ddof 1; 0 for one value)."""
    cnt, m, s, mean, m2 = 0, -np.inf, 0.0, 0.0, 0.0
    for k, mb, sb, meanb, m2b in parts:
        if k == 0:
            continue
        top = max(m, mb)
        s = s * np.exp(m - top) + sb * np.exp(mb - top)
        m = top
        tot, delta = cnt + k, meanb - mean          # Chan, Golub and LeVeque's pairwise merge
        mean += delta * (k / tot)
        m2 += m2b + delta * delta * (cnt * k / tot)
        cnt = tot
    return m + np.log(s) - np.log(cnt), (m2 / (cnt - 1) if cnt > 1 else 0.0)


def streamed(column, bounds):
    return merge_strips([walk_strip(column[a:b]) for a, b in bounds])


def _columns(rng, n):
    """Random log-likelihood columns as the kernel meets them: Bernoulli terms in (-5, 0), with some draws at the clamp log(tiny) ~ -87.3
    (a detection at z = 0) and some at -tiny (a non-detection there)."""
    cols = -rng.exponential(1.0, size=(n, 12))
    floor = np.log(np.float64(np.finfo(np.float32).tiny))      # -87.3365
    cols[:, 3:6] = np.where(rng.random((n, 3)) < 0.5, floor, cols[:, 3:6])
    cols[:, 6] = floor                                          # all equal: the variance is exactly 0
    cols[:, 7] = floor + rng.uniform(-0.05, 0.05, n)            # all near the floor
    cols[:, 8] = np.where(rng.random(n) < 0.5, -float(np.finfo(np.float32).tiny), cols[:, 8])
    cols[0, 9] = floor                                          # the floor first, then ordinary values: the maximum moves once
    return cols


@pytest.mark.parametrize("n, bounds", [
    (64, strip_bounds(64, 64)),                       # every strip of length 1
    (3, strip_bounds(3, 64)),                         # fewer draws than strips: lengths 1 and 0
    (1100, strip_bounds(1100, 64)),                   # 18 and 17
    (50, [(0, 1), (1, 1), (1, 20), (20, 21), (21, 50)]),   # unequal, a strip of length 1 and an empty one
    (2, [(0, 2)]),
], ids=["ones", "fewer_than_strips", "1100_in_64", "unequal", "one_strip"])
def test_streaming_merges_equal_logsumexp_and_var(n, bounds):
    assert bounds[0][0] == 0 and bounds[-1][1] == n and all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))
    cols = _columns(np.random.default_rng(n), n)
    for k in range(cols.shape[1]):
        lse, var = streamed(cols[:, k], bounds)
        want_lse, want_var = logsumexp(cols[:, k]) - np.log(n), np.var(cols[:, k], ddof=1)
        assert abs(lse - want_lse) <= 1e-12 * abs(want_lse) + 1e-13, (k, lse, want_lse)
        assert abs(var - want_var) <= 1e-12 * abs(want_var) + n * 2.0 ** -52 * 87.4 ** 2, (k, var, want_var)
    assert streamed(cols[:, 6], bounds)[1] == 0.0


def test_one_draw_has_variance_zero():
    lse, var = streamed(np.array([-87.3]), strip_bounds(1, 64))
    assert lse == -87.3 and var == 0.0


def test_strip_bounds_cover_the_draws_in_order():
    for n, R in [(1, 64), (63, 64), (64, 64), (65, 64), (1100, 64), (1000, 11), (7, 1)]:
        b = strip_bounds(n, R)
        assert len(b) == R and b[0][0] == 0 and b[-1][1] == n and all(x[1] == y[0] for x, y in zip(b, b[1:]))
        assert max(e - s for s, e in b) - min(e - s for s, e in b) <= 1
