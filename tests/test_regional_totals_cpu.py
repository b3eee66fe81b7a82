"""regional_totals without a GPU: the exports; the definition (tests/totals_ref.py) against the plainest loop; how labels become
regions -- strings, unsorted labels, ``None``, masked and NaN labels --; ``n_sites`` and ``weight``; the host's summaries against
NumPy's; every refusal and argument check of the wrapper that comes before a device is touched.

The definition against the loop: two float64 sums of the same terms, the bound derived in tests/totals_ref.py."""
import os
import re

import numpy as np
import pytest

import totals_ref
from biolith_amd import _ffi, models
from biolith_amd.utils import regional_totals
from biolith_amd.utils import regional_totals as _exported
from biolith_amd.utils.regional_totals import checked_weights, region_index, region_sizes, summarise, total_names

DATA = dict(site_covs=np.zeros((4, 1), np.float32), obs_covs=np.zeros((4, 1, 2, 1), np.float32), obs=np.zeros((1, 4, 1, 2), np.float32))
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "biolith_hip.h")


class _NoPosterior:
    """Any use of the posterior -- the first step towards a device -- fails the test."""

    def get_samples(self):
        raise AssertionError("the posterior was read: the refusal came too late")


def test_the_function_and_the_entry_are_exported():
    from biolith_amd import utils

    assert "regional_totals" in utils.__all__ and utils.regional_totals is _exported and callable(regional_totals)
    assert "bl_regional_totals" in _ffi.EXPORTS
    with open(HEADER) as f:
        header = f.read()
    assert re.search(r"\bint bl_regional_totals\(bl_dataset \*ds, int n_draws, const float \*draws, uint64_t seed, int n_regions,", header)
    assert "BL_TOTALS_WORKSPACE_BYTES" in header
    assert "np.einsum" in regional_totals.__doc__ and "conditional_occupancy" in regional_totals.__doc__
    assert total_names("occu") == total_names("occu_cs") == total_names("occu_cop") == ("psi", "z")
    assert total_names("occu_rn") == total_names("nmixture") == ("abundance", "N_i")


# ------------------------------------------------------------------------------------------ the definition ----
@pytest.mark.parametrize("weighted", [False, True], ids=["unit_weights", "weights"])
def test_the_definition_against_the_plainest_loop(weighted):
    rng = np.random.default_rng(0)
    n, N = 5, 211
    v = rng.random((n, N)).astype(np.float32)
    w = rng.normal(size=N) if weighted else None
    regions = rng.integers(0, 4, N).astype(np.float64)
    regions[rng.random(N) < 0.1] = np.nan
    labels, sites = totals_ref.region_sites(regions, N)
    assert np.array_equal(labels, [0.0, 1.0, 2.0, 3.0]) and sum(len(s) for s in sites) == int(np.isfinite(regions).sum())
    want, bound = totals_ref.totals(v[:, :, None], sites, w)
    loop = totals_ref.brute_force(v, sites, w)
    assert want.shape == (n, 4, 1) and np.all(np.abs(want[..., 0] - loop) <= bound[..., 0])
    z = rng.integers(0, 3, (n, N))   # integers with unit weights: exact
    assert np.array_equal(totals_ref.totals(z[:, :, None], sites)[0][..., 0], totals_ref.brute_force(z, sites))


# ------------------------------------------------------------------------------------------ labels ----
def test_string_labels_come_back_in_np_unique_order():
    lab = np.array(["wood", "fen", "wood", "moor", "fen", "wood"])
    labels, index = region_index(lab, 6)
    assert list(labels) == ["fen", "moor", "wood"] and index.dtype == np.int32 and list(index) == [2, 0, 2, 1, 0, 2]
    ref_labels, sites = totals_ref.region_sites(lab, 6)
    assert list(ref_labels) == list(labels) and [list(s) for s in sites] == [[1, 4], [3], [0, 2, 5]]


def test_unsorted_integer_and_bool_labels():
    labels, index = region_index(np.array([7, -3, 7, 100, -3]), 5)
    assert list(labels) == [-3, 7, 100] and list(index) == [1, 0, 1, 2, 0]
    labels, index = region_index(np.array([True, False, True]), 3)
    assert list(labels) == [False, True] and list(index) == [1, 0, 1]


def test_none_is_the_single_region_all():
    labels, index = region_index(None, 5)
    assert list(labels) == ["all"] and list(index) == [0] * 5
    assert list(totals_ref.region_sites(None, 5)[0]) == ["all"]


def test_masked_and_nan_labels_leave_the_site_out():
    lab = np.ma.masked_array(["b", "a", "b", "a"], mask=[False, True, False, False])
    labels, index = region_index(lab, 4)
    assert list(labels) == ["a", "b"] and list(index) == [1, -1, 1, 0]
    labels, index = region_index(np.array([2.0, np.nan, 1.0, 2.0]), 4)
    assert list(labels) == [1.0, 2.0] and list(index) == [1, -1, 0, 1]
    labels, index = region_index(np.ma.masked_array([2.0, np.nan, 1.0, 2.0], mask=[True, False, False, False]), 4)
    assert list(labels) == [1.0, 2.0] and list(index) == [-1, -1, 0, 1]
    # a label that no site in a region carries is no region
    labels, _ = region_index(np.ma.masked_array([5, 6, 7], mask=[False, True, False]), 3)
    assert list(labels) == [5, 7]
    with pytest.raises(ValueError, match="no site is in any region"):
        region_index(np.array([np.nan, np.nan]), 2)


def test_n_sites_and_weight():
    index = np.array([1, -1, 1, 0, 2, 1], dtype=np.int32)
    w = np.array([0.5, 100.0, -2.0, 3.0, 0.0, 1.25])
    counts, weight = region_sizes(index, w, 3)
    assert counts.dtype == np.int64 and list(counts) == [1, 3, 1] and weight.dtype == np.float64 and list(weight) == [3.0, -0.25, 0.0]
    counts, weight = region_sizes(index, None, 3)
    assert list(counts) == [1, 3, 1] and list(weight) == [1.0, 3.0, 1.0]


# ------------------------------------------------------------------------------------------ the host's summaries ----
@pytest.mark.parametrize("n", [1, 2, 100])
def test_summaries_against_numpy(n):
    d = np.random.default_rng(n).normal(size=(n, 2, 3, 1))
    probs = np.array([0.0, 0.05, 0.5, 1.0 / 3.0, 1.0])
    s = summarise(d, probs)
    assert s["draws"] is d and set(s) == {"draws", "mean", "sd", "quantiles"}
    assert np.array_equal(s["mean"], np.mean(d, axis=0)) and np.array_equal(s["quantiles"], np.quantile(d, probs, axis=0))
    assert s["quantiles"].shape == (5, 2, 3, 1) and s["sd"].shape == (2, 3, 1)
    if n == 1:
        assert np.isnan(s["sd"]).all()
    else:
        assert np.array_equal(s["sd"], np.std(d, axis=0, ddof=1))
    totals_ref.check_summaries(s, probs)


# ------------------------------------------------------------------------------------------ refusals before any device call ----
@pytest.mark.parametrize("name", ["occu_comb", "occu_dyn"])
def test_models_whose_sites_are_formed_on_the_host_are_refused(name):
    with pytest.raises(NotImplementedError, match=rf"regional_totals\(\): not built for {name} .*predict\(\) followed by"):
        regional_totals(getattr(models, name), _NoPosterior(), **DATA)


def test_not_a_model_is_a_type_error():
    with pytest.raises(TypeError, match="biolith_amd model"):
        regional_totals(lambda **kw: None, _NoPosterior(), **DATA)
    with pytest.raises(TypeError, match="biolith_amd model"):
        regional_totals("occu", _NoPosterior(), **DATA)


@pytest.mark.parametrize("probs,message", [((), "empty"), ((0.5, 1.5), r"\[0, 1\]"), ((-0.1,), r"\[0, 1\]"), ((np.nan,), r"\[0, 1\]")])
def test_bad_probs_are_value_errors(probs, message):
    with pytest.raises(ValueError, match=message):
        regional_totals(models.occu, _NoPosterior(), **DATA, probs=probs)


def test_regions_or_weights_of_the_wrong_length_are_value_errors():
    with pytest.raises(ValueError, match="`regions` holds 3 labels for 4 sites"):
        regional_totals(models.occu, _NoPosterior(), **DATA, regions=[0, 1, 0])
    with pytest.raises(ValueError, match="`weights` holds 5 values for 4 sites"):
        regional_totals(models.occu, _NoPosterior(), **DATA, weights=np.ones(5))
    with pytest.raises(ValueError, match="`weights` holds 5 values for 4 sites"):
        checked_weights(np.ones(5), 4)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_weight_is_a_value_error(bad):
    w = np.array([1.0, 2.0, bad, 4.0])
    with pytest.raises(ValueError, match=r"weights\[2\]=.* is not finite"):
        regional_totals(models.occu, _NoPosterior(), **DATA, weights=w)
    assert checked_weights(None, 4) is None and checked_weights([0.0, -1.0, 2, 3], 4).dtype == np.float64
