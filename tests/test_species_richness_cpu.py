"""species_richness without a GPU: the definition (tests/richness_ref.py) against the enumeration of all 2^S presence patterns in exact
rational arithmetic for S <= 10 and against its identities -- rows sum to 1, ``sum r pi = sum p``, the species' order moves the pmf
only within the bound, a species with p = 0 leaves and one with p = 1 shifts the pmf exactly --; the area sum's order against the
plain sum; the integer quantile rule on hand-made pmfs; the exports; every refusal of the wrapper that comes before a device is
touched.  The bounds are the ones derived in tests/richness_ref.py; the largest error seen is printed as a fraction of them."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import richness_ref
from biolith_amd import _ffi, models

U = richness_ref.U
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "biolith_hip.h")
DATA = dict(site_covs=np.zeros((4, 1), np.float32), obs_covs=np.zeros((4, 1, 2, 1), np.float32), obs=np.zeros((2, 4, 1, 2), np.float32))


def _psi(rng, shape, edges=False):
    """float32 probabilities as a sigmoid of coefficients in (-1, 1) on standard-normal covariates gives them; with ``edges`` some are
    exactly 0 or 1."""
    eta = rng.uniform(-1, 1, shape) + rng.normal(size=shape) * rng.uniform(-1, 1, shape)
    psi = (1.0 / (1.0 + np.exp(-eta))).astype(np.float32)
    if edges:
        pick = rng.random(shape)
        psi[pick < 0.1], psi[pick > 0.9] = 0.0, 1.0
    return psi


# ------------------------------------------------------------------------------------------ the definition ----
@pytest.mark.parametrize("S", [1, 2, 3, 7, 10])
@pytest.mark.parametrize("edges", [False, True], ids=["inside", "with_0_and_1"])
def test_the_recursion_against_the_enumeration_of_all_patterns(S, edges):
    rng = np.random.default_rng(S)
    psi = _psi(rng, (6, S), edges)
    pi, E = richness_ref.pmf(psi)
    worst = 0.0
    for k in range(6):
        exact = richness_ref.enumerate_pmf(psi[k])
        assert sum(exact) == 1
        for r in range(S + 1):
            err = abs(Fraction(float(pi[k, r])) - exact[r])
            assert err <= Fraction(4 * S) * Fraction(U) * exact[r], (S, k, r)
            if exact[r]:
                worst = max(worst, float(err / (Fraction(4 * S) * Fraction(U) * exact[r])))
        assert abs(Fraction(float(E[k])) - sum(Fraction(float(v)) for v in psi[k])) <= Fraction(max(S - 1, 0)) * Fraction(U) * Fraction(float(E[k]))
    print(f"S={S} edges={edges}: largest error {worst:.3g} of 4 S u")


@pytest.mark.parametrize("S", [1, 5, 16, 32])
def test_the_identities(S):
    rng = np.random.default_rng(100 + S)
    psi = _psi(rng, (40, S))
    pi, E = richness_ref.pmf(psi)
    richness_ref.assert_scaled(pi)
    assert pi.shape == (40, S + 1) and np.all(pi >= 0)
    # rows sum to 1, sum r pi = sum p: sums of S + 1 entries each within 4 S u, and the sum's own rounding
    assert np.all(np.abs(pi.sum(-1) - 1.0) <= (4 * S + S) * U)
    first = pi @ np.arange(S + 1)
    assert np.all(np.abs(first - E) <= (4 * S + 2 * S) * U * E)
    # the species' order: two evaluations of the same pmf
    order = rng.permutation(S)
    other, E2 = richness_ref.pmf(psi[:, order])
    err, bound = np.abs(other - pi), 8 * S * U * pi
    assert np.all(err <= bound) and np.all(np.abs(E2 - E) <= 2 * (S - 1) * U * E)
    print(f"S={S}: the species' order moves the pmf by at most {float(np.max(err / bound)):.3g} of 8 S u")


def test_a_species_with_p_0_leaves_and_one_with_p_1_shifts_the_pmf_exactly():
    rng = np.random.default_rng(7)
    psi = _psi(rng, (30, 6))
    pi, E = richness_ref.pmf(psi)
    for at in (0, 3, 6):   # in front, in the middle, behind
        for value, shift in ((0.0, 0), (1.0, 1)):
            more = np.insert(psi, at, np.float32(value), axis=-1)
            got, E_more = richness_ref.pmf(more)
            want = np.zeros((30, 8))
            want[:, shift:shift + 7] = pi
            if at == 6 or value == 0.0 or at == 0:
                # p = 0 anywhere, and p = 1 at either end, are exact: every product is by 1.0 or 0.0
                assert got.tobytes() == want.tobytes(), (at, value)
            else:
                assert np.all(np.abs(got - want) <= 8 * 7 * U * want), (at, value)
            if value == 0.0:
                assert E_more.tobytes() == E.tobytes()


def test_the_area_sum_in_the_devices_order_against_the_plain_sum():
    rng = np.random.default_rng(8)
    n, N, S = 3, 300, 4
    pi, _ = richness_ref.pmf(_psi(rng, (n, N, S)))
    w = rng.normal(size=N)
    lab = rng.integers(0, 3, N)
    sites = [np.flatnonzero(lab == g) for g in range(3)] + [np.arange(0)]
    got, bound = richness_ref.area(pi, sites, w)
    assert got.shape == (n, S + 1, 4) and not got[..., 3].any()
    for g in range(3):
        plain = np.einsum("i,nir->nr", w[sites[g]], pi[:, sites[g]])
        assert np.all(np.abs(got[..., g] - plain) <= bound[..., g])
    # one site: the term's bits; the tree on a run by hand
    one, _ = richness_ref.area(pi, [np.array([5])], w)
    assert one[..., 0].tobytes() == (w[5] * pi[:, 5]).tobytes()
    x = rng.normal(size=64)
    a = x[:32] + x[32:]
    b = a[:16] + a[16:]
    c = b[:8] + b[8:]
    d = c[:4] + c[4:]
    e = d[:2] + d[2:]
    assert richness_ref.wave_tree(x) == e[0] + e[1]


def test_the_site_sums_run_in_draw_order():
    rng = np.random.default_rng(9)
    psi = _psi(rng, (5, 3, 4))
    pmf_mean, e_mean, e_sd = richness_ref.site_outputs(psi)
    pi, E = richness_ref.pmf(psi)
    want = ((((pi[0] + pi[1]) + pi[2]) + pi[3]) + pi[4]) / 5
    assert pmf_mean.tobytes() == want.tobytes()
    assert e_mean.tobytes() == (((((E[0] + E[1]) + E[2]) + E[3]) + E[4]) / 5).tobytes()
    assert np.allclose(e_sd, E.std(axis=0, ddof=1), rtol=1e-12)
    assert np.isnan(richness_ref.site_outputs(psi[:1])[2]).all()


# ------------------------------------------------------------------------------------------ the wrapper's host side ----
def test_the_function_and_the_entry_are_exported():
    from biolith_amd import utils
    from biolith_amd.utils.species_richness import species_richness

    assert "species_richness" in utils.__all__ and utils.species_richness is species_richness
    assert "bl_species_richness" in _ffi.EXPORTS and _ffi.RICHNESS_MAX_SPECIES == 32
    with open(HEADER) as f:
        header = f.read()
    assert re.search(r"\bint bl_species_richness\(bl_dataset \*ds, int n_species, int n_draws, const float \*draws", header)
    assert re.search(r"#define BL_RICHNESS_MAX_SPECIES 32\b", header)
    assert "conditional_occupancy" in species_richness.__doc__


def test_the_integer_quantile_rule():
    from biolith_amd.utils.species_richness import pmf_quantiles

    pmf = np.array([[0.5, 0.25, 0.25], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.05, 0.9, 0.05], [0.3, 0.3, 0.3]])   # (the last sums to 0.9)
    probs = np.array([0.0, 0.05, 0.5, 0.75, 0.95, 1.0])
    got = pmf_quantiles(pmf, probs)
    # (q = 0: cumsum >= 0 at r = 0 whatever the pmf)
    want = np.array([[0, 0, 0, 0, 0], [0, 2, 0, 0, 0], [0, 2, 0, 1, 1], [1, 2, 0, 1, 2], [2, 2, 0, 1, 2], [2, 2, 0, 2, 2]])
    assert got.dtype == np.int64 and np.array_equal(got, want), got
    assert np.array_equal(got, richness_ref.integer_quantiles(pmf, probs))
    rng = np.random.default_rng(3)
    rows = rng.dirichlet(np.ones(9), size=(4, 5))
    assert np.array_equal(pmf_quantiles(rows, [0.1, 0.5, 0.9]), richness_ref.integer_quantiles(rows, [0.1, 0.5, 0.9]))


class _NoPosterior:
    """Any use of the posterior -- the first step towards a device -- fails the test."""

    def get_samples(self):
        raise AssertionError("the posterior was read: the refusal came too late")


class _Posterior:
    def __init__(self, sites):
        self.sites = sites

    def get_samples(self):
        return self.sites


def _sites(n=3, S=2, Ks=1, Ko=1):
    rng = np.random.default_rng(0)
    return dict(beta=rng.uniform(-1, 1, (n, S, Ks + 1)).astype(np.float32), alpha=rng.uniform(-1, 1, (n, S, Ko + 1)).astype(np.float32))


@pytest.fixture
def no_device(monkeypatch):
    """Opening a handle fails the test: every refusal below is decided on the host."""
    import importlib

    def refuse(*a, **k):
        raise AssertionError("a handle was opened: the refusal came too late")

    # (the package's attribute of this name is the function; the module is under its dotted name)
    monkeypatch.setattr(importlib.import_module("biolith_amd.utils.species_richness"), "species_dataset", refuse)


def test_refusals_before_the_device(no_device):
    from biolith_amd.utils import species_richness

    with pytest.raises(TypeError, match="biolith_amd model"):
        species_richness(lambda **k: None, _NoPosterior(), **DATA)
    with pytest.raises(TypeError):
        species_richness("occu", _NoPosterior(), **DATA)
    for name in ("occu_rn", "nmixture", "occu_cop", "occu_cs", "occu_comb", "occu_dyn"):
        with pytest.raises(NotImplementedError, match="one species per call"):
            species_richness(getattr(models, name), _NoPosterior(), **DATA)
    for probs in ((), (0.5, 1.5), (-0.1,)):
        with pytest.raises(ValueError):
            species_richness(models.occu, _NoPosterior(), **DATA, probs=probs)
    with pytest.raises(ValueError, match="labels for 4 sites"):
        species_richness(models.occu, _NoPosterior(), **DATA, regions=np.arange(3))
    with pytest.raises(ValueError, match="no site is in any region"):
        species_richness(models.occu, _NoPosterior(), **DATA, regions=np.full(4, np.nan))
    with pytest.raises(ValueError, match="values for 4 sites"):
        species_richness(models.occu, _NoPosterior(), **DATA, weights=np.ones(5))
    with pytest.raises(ValueError, match=r"weights\[2\]=inf is not finite"):
        species_richness(models.occu, _NoPosterior(), **DATA, weights=np.array([1.0, 1.0, np.inf, 1.0]))
    # the posterior
    with pytest.raises(ValueError, match="no draws"):
        species_richness(models.occu, _Posterior(_sites(n=0)), **DATA)
    with pytest.raises(ValueError, match="33 species, at most 32"):
        species_richness(models.occu, _Posterior(_sites(S=33)), **DATA)
    with pytest.raises(ValueError, match="covariate counts differ"):
        species_richness(models.occu, _Posterior(_sites(Ks=2)), **DATA)
    with pytest.raises(ValueError, match="covariate counts differ"):
        species_richness(models.occu, _Posterior(_sites(Ko=3)), **DATA)
    for bad in (np.nan, np.inf):
        sites = _sites()
        sites["beta"][1, 1, 0] = bad
        with pytest.raises(ValueError, match="non-finite draws"):
            species_richness(models.occu, _Posterior(sites), **DATA)
    # ... and a posterior that passes every check reaches the handle
    with pytest.raises(AssertionError, match="a handle was opened"):
        species_richness(models.occu, _Posterior(_sites()), **DATA)
