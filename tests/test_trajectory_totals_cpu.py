"""trajectory_totals without a GPU: the NumPy definition (tests/trajectory_ref.py) against the enumeration of a site's 2^T paths and its
own identities, its restatement of the device's summation order, and every refusal of the wrapper that is decided before the device is
touched.  (The wrapper is imported where it is used: the definition's own checks need nothing of it.)"""
import warnings

import numpy as np
import pytest

import trajectory_ref as ref
from biolith_amd import models

f32 = lambda a: np.asarray(a, dtype=np.float32)


class _Posterior:
    def __init__(self, sites):
        self.sites = sites

    def get_samples(self):
        return self.sites


def _case(seed, N=9, n=3, Ks=2, Ko=1):
    rng = np.random.default_rng(seed)
    X = f32(rng.normal(size=(N, Ks)))
    sites = {k: f32(rng.uniform(-1, 1, (n, 1, Ks + 1))) for k in ref.BLOCKS}
    sites["alpha"] = f32(rng.uniform(-1, 1, (n, 1, Ko + 1)))
    return X, sites


# ------------------------------------------------------------------------------------------ the definition ----
@pytest.mark.parametrize("T", [1, 2, 3, 4])
def test_the_recursion_is_the_sum_over_the_paths(T):
    X, sites = _case(T, N=5, n=2)
    psi, gam, eps, _ = ref.rates(X, sites)
    values, bounds = ref.expected(X, sites, T)
    for n in range(2):
        for i in range(5):
            pi, col, ext = ref.brute_force(psi[n, i], gam[n, i], eps[n, i], T)
            # 2^T products of T factors, summed: T + 2^T roundings of values <= 1 on that side, the recursion's bound on this one
            slack = (T + 2 ** T) * ref.U
            assert np.all(np.abs(values["occupancy"][n, :, i] - pi) <= bounds["occupancy"][n, :, i] + slack)
            assert np.all(np.abs(values["colonised"][n, :, i] - col) <= bounds["colonised"][n, :, i] + slack)
            assert np.all(np.abs(values["extinct"][n, :, i] - ext) <= bounds["extinct"][n, :, i] + slack)
    assert values["colonised"].shape == values["extinct"].shape == (2, T - 1, 5) and values["equilibrium"].shape == (2, 5)


def test_the_realised_path_follows_its_uniforms():
    """The path's frequencies over many draws approach the recursion (the generator is exact: tests/test_pred_rng_ref_cpu.py), and its
    transitions are the differences of its states."""
    X, sites = _case(10, N=4, n=1)
    many = {k: np.repeat(v, 4000, axis=0) for k, v in sites.items()}
    z, near = ref.path(X, many, 4, seed=3)
    assert near == 0
    values, _ = ref.expected(X, many, 4)
    assert np.all(np.abs(z.mean(axis=0) - values["occupancy"][0]) < 5 * 0.5 / np.sqrt(4000))
    r = ref.realised(z)
    assert np.array_equal(r["z"][:, 1:] - r["z"][:, :-1], r["z_colonised"] - r["z_extinct"])
    assert not (r["z_colonised"] * r["z_extinct"]).any()
    assert np.abs(r["z_colonised"].mean(axis=0) - values["colonised"][0]).max() < 5 * 0.5 / np.sqrt(4000)
    # a later first draw continues the same stream of cells
    z2, _ = ref.path(X, {k: v[5:9] for k, v in many.items()}, 4, seed=3, first_draw=5)
    assert np.array_equal(z2, z[5:9])
    assert not np.array_equal(ref.path(X, many, 4, seed=4)[0], z)
    assert not np.array_equal(ref.path(X, many, 5, seed=3)[0][:, :4], z)   # the cell's index holds T


def test_growth_rate_and_turnover_identities():
    X, sites = _case(11, N=40, n=3, Ks=3)
    values, _ = ref.expected(X, sites, 5)
    w = np.random.default_rng(1).uniform(0.5, 2.0, 40)
    occ, col, ext = (np.sum(w * values[k], axis=-1) for k in ("occupancy", "colonised", "extinct"))
    # the balance of a season: what is occupied next is what was, less what was lost, plus what was gained
    assert np.allclose(occ[:, 1:], occ[:, :-1] - ext + col, rtol=1e-13, atol=0)
    g, tv = ref.growth_rate(occ), ref.turnover(col, occ)
    assert g.shape == tv.shape == (3, 4)
    assert np.allclose(g, 1.0 + (col - ext) / occ[:, :-1], rtol=1e-13, atol=0)
    assert np.all(tv > 0) and np.all(tv < 1)          # colonised_t is a part of occupancy_t+1
    # at the equilibrium nothing moves: started there, the occupancy stays and the growth rate is 1
    psi, gam, eps, _ = ref.rates(X, sites)
    eq = values["equilibrium"]
    assert np.allclose(eq * (1.0 - eps) + (1.0 - eq) * gam, eq, rtol=1e-14, atol=0)
    # a zero denominator is NaN, and silent
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        z = np.zeros((2, 3))
        assert np.isnan(ref.growth_rate(z)).all() and np.isnan(ref.turnover(z[:, 1:], z)).all()
        one = np.array([[0.0, 2.0, 4.0]])
        assert np.array_equal(ref.growth_rate(one), [[np.nan, 2.0]], equal_nan=True)
    assert ref.growth_rate(occ[:, :1]).shape == (3, 0)


def test_ordered_sum_is_a_sum_in_one_fixed_order():
    rng = np.random.default_rng(12)
    for N in (1, 2, 63, 64, 65, 130, 300):
        t = rng.normal(size=(3, N)) * 10.0 ** rng.integers(-3, 4, N)
        s = ref.ordered_sum(t)
        assert s.shape == (3,)
        assert np.all(np.abs(s - np.sum(t, axis=-1)) <= 2 * max(N - 1, 0) * ref.U * np.abs(t).sum(axis=-1)), N
    assert ref.ordered_sum(np.array([-3.25])).tobytes() == np.array(-3.25).tobytes()      # one site: its term's bits
    assert np.signbit(ref.ordered_sum(np.array([-0.0])))                                 # -0.0 is the identity
    ints = rng.integers(0, 2, (4, 200)).astype(np.float64)
    assert np.array_equal(ref.ordered_sum(ints), ints.sum(axis=-1))
    assert ref.ordered_sum(np.empty((2, 0))).tolist() == [0.0, 0.0]


# ------------------------------------------------------------------------------------------ the wrapper's front ----
def test_import_and_all():
    import biolith_amd.utils as utils
    from biolith_amd.utils.trajectory_totals import trajectory_totals

    assert utils.trajectory_totals is trajectory_totals and "trajectory_totals" in utils.__all__
    assert "share a distribution and NOT their values" in " ".join(trajectory_totals.__doc__.split())   # (predict()'s z: the host's generator)


def test_refusals_before_the_device():
    from biolith_amd.utils import trajectory_totals

    X, sites = _case(20, N=12)
    post = _Posterior(sites)
    W = np.zeros((12, 3, 2, 1), dtype=np.float32)
    call = lambda model=models.occu_dyn, posterior=post, **kw: trajectory_totals(model, posterior, **{"site_covs": X, "obs_covs": W, **kw})
    with pytest.raises(TypeError, match="must be a biolith_amd model"):
        call(model=lambda **kw: None)
    with pytest.raises(TypeError):
        call(model="occu_dyn")
    for name in ("occu", "occu_rn", "occu_cop", "occu_cs", "nmixture", "occu_comb"):
        with pytest.raises(NotImplementedError, match=f"not built for {name} "):
            call(model=getattr(models, name))
    for bad in (0, -3):
        with pytest.raises(ValueError, match=f"n_periods={bad}"):
            call(n_periods=bad)
    with pytest.raises(ValueError, match="n_periods"):
        call(obs_covs=None)
    with pytest.raises(ValueError, match="`regions` holds 5 labels for 12 sites"):
        call(regions=np.arange(5))
    with pytest.raises(ValueError, match="`weights` holds 3 values for 12 sites"):
        call(weights=np.ones(3))
    w = np.ones(12)
    for bad in (np.nan, np.inf):
        w[7] = bad
        with pytest.raises(ValueError, match=r"weights\[7\]"):
            call(weights=w)
    with pytest.raises(ValueError, match="no site is in any region"):
        call(regions=np.full(12, np.nan))
    with pytest.raises(ValueError, match="no site is in any region"):
        call(regions=np.ma.masked_all(12, dtype=int))
    with pytest.raises(ValueError, match="covariate counts differ"):
        call(site_covs=X[:, :1])
    with pytest.raises(ValueError, match="covariate counts differ"):
        call(obs_covs=np.zeros((12, 3, 2, 2), dtype=np.float32))
    with pytest.raises(ValueError, match="covariate counts differ"):
        call(posterior=_Posterior({**sites, "beta_ext": sites["beta_ext"][:, :, :2]}))
    with pytest.raises(ValueError, match="holds no draws"):
        call(posterior=_Posterior({k: v[:0] for k, v in sites.items()}))
    with pytest.raises(ValueError, match="several species"):
        call(posterior=_Posterior({k: np.repeat(v, 2, axis=1) for k, v in sites.items()}))
    with pytest.raises(ValueError, match="obs_covs holds 5 sites"):
        call(obs_covs=W[:5])
    for bad in ((), (0.5, 1.5)):
        with pytest.raises(ValueError):
            call(probs=bad)
    with pytest.raises(NotImplementedError, match="coords"):
        call(coords=np.zeros((12, 2)))


def test_the_siblings_still_refuse_occu_dyn():
    from biolith_amd.utils import regional_totals, response_curves, site_diagnostics, site_summary

    X, sites = _case(21, N=12)
    W = np.zeros((12, 3, 2, 1), dtype=np.float32)
    for fn in (site_summary, site_diagnostics, regional_totals, response_curves):
        with pytest.raises(NotImplementedError, match=r"not built for occu_dyn \(its sites are formed on the host\)"):
            fn(models.occu_dyn, _Posterior(sites), site_covs=X, obs_covs=W)
