"""trajectory_totals on the GPU: the fused totals of an occu_dyn posterior's occupancy over the seasons (bl_trajectory_totals) against
their definition in NumPy float64 (tests/trajectory_ref.py): the geometry (one site, sizes around a wave and a block, one, two and five
seasons, one, two and eight covariates, interleaved and masked labels, a draw loop that strides past the grid rows, a chunk boundary);
every site its own region, where a total is one term; zero, negative and unit weights; the locality of a region's rows; the same bytes
twice, from each output alone, under another seed, from the first draws and from another handle of the same sites; the forecast;
``obs_covs=None``; the host path's psi; a small real fit; the refusals at the C-ABI.

Posteriors are hand-made (random float32 coefficients in (-1, 1) behind a ``get_samples()`` stub); one fit of 60 sites, 100 + 100
draws.  The expected totals are within the derived bound of trajectory_ref's docstring, which ``check`` asserts is below
1e-12 sum |w|; the realised totals are EQUAL to the restatement, whose count of cells at a threshold every comparison asserts is 0."""
import contextlib
import ctypes as C
import io
import warnings

import numpy as np
import pytest

import trajectory_ref as ref
from biolith_amd import _ffi, models
from biolith_amd.engine import OccuDataset
from biolith_amd.models import simulate_dyn
from biolith_amd.utils import fit, predict, trajectory_totals

pytestmark = pytest.mark.gpu

PROBS = (0.05, 0.5, 0.95)
NAMES = OccuDataset.TRAJECTORY_OUTPUTS
f32 = lambda a: np.asarray(a, dtype=np.float32)


class _Posterior:
    """What predict and trajectory_totals read of a fit: ``get_samples()``."""

    def __init__(self, sites):
        self.sites = sites

    def get_samples(self):
        return self.sites


def _case(seed, N=70, n=3, Ks=2, Ko=1):
    """Random site covariates and a hand-made posterior for them (coefficients in (-1, 1))."""
    rng = np.random.default_rng(seed)
    X = f32(rng.normal(size=(N, Ks)))
    sites = {k: f32(rng.uniform(-1, 1, (n, 1, Ks + 1))) for k in ref.BLOCKS}
    sites["alpha"] = f32(rng.uniform(-1, 1, (n, 1, Ko + 1)))
    return X, _Posterior(sites)


def _handle(X, posterior, T=1, J=1, obs=None):
    """A handle of the sites with T x J visits (all masked unless ``obs``) and the posterior's draw matrix [b_psi | b_col | b_ext | alpha]."""
    s = posterior.sites
    Ko = s["alpha"].shape[2] - 1
    Y = np.full((1, X.shape[0], T, J), np.nan, dtype=np.float32) if obs is None else obs
    ds = OccuDataset(X, np.zeros((X.shape[0], T, J, Ko), dtype=np.float32), Y, model="occu_dyn")
    return ds, np.ascontiguousarray(np.concatenate([s[k][:, 0] for k in ref.BLOCKS + ("alpha",)], axis=1))


def _compare(X, posterior, T, regions=None, weights=None, seed=0, label="", **more):
    got = trajectory_totals(models.occu_dyn, posterior, site_covs=X, n_periods=T, regions=regions, weights=weights, probs=PROBS,
                            random_seed=seed, **more)
    worst = ref.check(got, X, posterior.sites, T, regions, weights, PROBS, seed, more.get("latent", True), label)
    print(f"{label}: largest error {worst:.3g} of its bound")
    return got


def _interleaved(N, seed=0):
    """Labels of N >= 256 sites in no order: regions of 1, 63, 64 and 65 sites and one of the remainder."""
    lab = np.repeat(np.array(["one", "w63", "w64", "w65", "rest"]), [1, 63, 64, 65, N - 193])
    return np.random.default_rng(seed).permutation(lab)


# ------------------------------------------------------------------------------------------ geometry ----
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 300])
@pytest.mark.parametrize("n", [1, 3])
def test_one_region(N, n):
    X, posterior = _case(N, N=N, n=n)
    w = np.random.default_rng(N).uniform(0.1, 5.0, N)
    got = _compare(X, posterior, 5, weights=w, seed=N, label=f"N={N} n={n}")
    assert list(got["regions"]) == ["all"] and got["occupancy"]["draws"].shape == (n, 5, 1, 1)
    if n == 1:
        assert all(np.isnan(got[k]["sd"]).all() for k in ("occupancy", "equilibrium", "turnover", "z_extinct"))


@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("Ks", [1, 2, 8])
def test_periods_and_covariates(T, Ks):
    X, posterior = _case(100 + 10 * T + Ks, N=257, n=3, Ks=Ks)
    lab = np.random.default_rng(Ks).integers(0, 3, 257)
    got = _compare(X, posterior, T, regions=lab, weights=np.linspace(0.5, 2.0, 257), seed=T, label=f"T={T} Ks={Ks}")
    assert got["colonised"]["draws"].shape == got["turnover"]["draws"].shape == got["z_extinct"]["draws"].shape == (3, T - 1, 3, 1)
    assert got["equilibrium"]["quantiles"].shape == (3, 3, 1) and got["z"]["mean"].shape == (T, 3, 1)


def test_no_site_covariates_and_missing_ones():
    X, posterior = _case(7, N=70, Ks=0)
    _compare(X, posterior, 3, label="Ks=0")
    X, posterior = _case(8, N=70, Ks=2)
    X[::7, 1] = np.nan                                  # NaN -> 0, as the fit packs it
    _compare(X, posterior, 3, label="NaN covariates")


@pytest.mark.parametrize("n", [1, 3])
def test_interleaved_and_masked_labels(n):
    X, posterior = _case(11, N=300, n=n)
    lab = _interleaved(300)
    assert not np.array_equal(lab, np.sort(lab))
    w = np.random.default_rng(1).uniform(0.1, 5.0, 300)
    got = _compare(X, posterior, 5, regions=lab, weights=w, seed=2, label=f"interleaved n={n}")
    assert list(got["regions"]) == ["one", "rest", "w63", "w64", "w65"] and list(got["n_sites"]) == [1, 107, 63, 64, 65]
    _compare(X, posterior, 5, regions=lab, seed=2, label=f"interleaved, unit weights n={n}")
    out = np.ma.masked_array(lab, mask=lab == "w64")
    less = _compare(X, posterior, 5, regions=out, weights=w, seed=2, label=f"a masked label n={n}")
    assert list(less["regions"]) == ["one", "rest", "w63", "w65"]
    for k in NAMES:
        assert np.ascontiguousarray(less[k]["draws"][..., 3, :]).tobytes() == np.ascontiguousarray(got[k]["draws"][..., 4, :]).tobytes(), k


def test_the_draw_loop_strides_past_the_grid_rows():
    X, posterior = _case(12, N=40, n=1100)
    lab = np.random.default_rng(2).integers(0, 3, 40)
    _compare(X, posterior, 2, regions=lab, weights=np.linspace(-1.0, 2.0, 40), seed=1, label="n=1100")


def test_a_chunk_boundary():
    """One region per site at N = 11 000 and T = 3: 11 000 waves x 15 output rows x 8 bytes a draw, so 203 draws fill the 256 MB of the
    workspace and the 220 draws go through in two chunks.  Every total is one term; 400 of the sites, the first and the last among
    them, are compared with the definition over all the draws."""
    N, n, T = 11000, 220, 3
    X, posterior = _case(13, N=N, n=n)
    ds, draws = _handle(X, posterior)
    w = np.random.default_rng(3).normal(size=N)
    res = ds.trajectory_totals(draws, np.arange(N), N, T, weight=w, seed=5)
    ds.close()
    pick = np.unique(np.concatenate([[0, 63, 64, N - 1], np.random.default_rng(4).integers(0, N, 400)]))
    ref.check_terms({k: v[..., pick] for k, v in res.items()}, X[pick], posterior.sites, T, w[pick], 5, of=(pick, N))


# ------------------------------------------------------------------------------------------ every site its own region ----
@pytest.mark.parametrize("Ks", [1, 2, 8])
def test_every_site_its_own_region(Ks):
    """Unit weights: the draws are the terms themselves, each within the per-term bound -- the arithmetic apart from the summation."""
    X, posterior = _case(30 + Ks, N=65, Ks=Ks)
    got = _compare(X, posterior, 5, regions=np.arange(65), seed=9, label=f"own region Ks={Ks}")
    assert list(got["n_sites"]) == [1] * 65 and np.array_equal(got["weight"], np.ones(65))
    ref.check_terms({k: got[k]["draws"][..., 0] for k in NAMES}, X, posterior.sites, 5, np.ones(65), 9)
    occ = got["occupancy"]["draws"]
    assert np.all(occ > 0) and np.all(occ < 1) and set(np.unique(got["z"]["draws"])) == {0.0, 1.0}


# ------------------------------------------------------------------------------------------ weights ----
def test_zero_negative_and_unit_weights():
    X, posterior = _case(60, N=130)
    lab = np.random.default_rng(61).integers(0, 2, 130)
    run = lambda w: trajectory_totals(models.occu_dyn, posterior, site_covs=X, n_periods=4, regions=lab, weights=w, probs=PROBS, random_seed=2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                   # 0 / 0 is NaN, and silent
        zero = run(np.zeros(130))
    assert all(not zero[k]["draws"].any() for k in NAMES) and list(zero["weight"]) == [0.0, 0.0]
    assert np.isnan(zero["growth_rate"]["draws"]).all() and np.isnan(zero["turnover"]["draws"]).all()
    unit, ones = run(None), run(np.ones(130))
    for k in NAMES + ("growth_rate", "turnover"):
        assert unit[k]["draws"].tobytes() == ones[k]["draws"].tobytes(), k
    for k in ref.REALISED:   # integers
        assert np.array_equal(unit[k]["draws"], np.round(unit[k]["draws"])), k
    z = unit["z"]["draws"]
    assert np.array_equal(z[:, 1:] - z[:, :-1], unit["z_colonised"]["draws"] - unit["z_extinct"]["draws"])
    minus = run(-np.ones(130))
    for k in ref.REALISED:
        assert np.array_equal(minus[k]["draws"], -unit[k]["draws"]), k
    assert np.all(minus["occupancy"]["draws"] < 0) and np.all(minus["growth_rate"]["draws"] > 0)
    _compare(X, posterior, 4, regions=lab, seed=2, label="unit weights")
    _compare(X, posterior, 4, regions=lab, weights=np.linspace(-2.0, 1.0, 130), seed=2, label="negative weights")


# ------------------------------------------------------------------------------------------ locality ----
def test_a_regions_rows_do_not_depend_on_the_other_sites_labels():
    N = 300
    X, posterior = _case(50, N=N)
    rng = np.random.default_rng(51)
    w = rng.uniform(-1.0, 3.0, N)
    in_a = rng.random(N) < 0.4
    others = np.flatnonzero(~in_a)
    one = np.where(in_a, "A", "B")
    three = one.copy()
    three[others] = np.array(["B", "C", "D"])[rng.integers(0, 3, others.size)]
    out = np.ma.masked_array(one, mask=~in_a)
    run = lambda lab: trajectory_totals(models.occu_dyn, posterior, site_covs=X, n_periods=4, regions=lab, weights=w, probs=PROBS, random_seed=6)
    a, b, c = run(one), run(three), run(out)
    assert list(a["regions"]) == ["A", "B"] and list(b["regions"]) == ["A", "B", "C", "D"] and list(c["regions"]) == ["A"]
    for k in NAMES + ("growth_rate", "turnover"):
        rows = [np.ascontiguousarray(r[k]["draws"][..., 0, :]).tobytes() for r in (a, b, c)]
        assert rows[0] == rows[1] == rows[2], k


# ------------------------------------------------------------------------------------------ determinism and outputs ----
def _abi(ds, draws, region, G, T, weight=None, seed=0, which=range(7)):
    """bl_trajectory_totals through ctypes with only the outputs ``which`` passed; the others stay untouched (-7)."""
    n = draws.shape[0]
    r32 = np.ascontiguousarray(region, dtype=np.int32)
    g, pairs = max(G, 1), max(T - 1, 0)
    out = [np.full(s, -7.0) for s in ((n, max(T, 0), g), (n, pairs, g), (n, pairs, g), (n, g), (n, max(T, 0), g), (n, pairs, g), (n, pairs, g))]
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    rc = ds._lib.bl_trajectory_totals(ds._h, n, draws.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint64(seed), T, G,
                                      r32.ctypes.data_as(C.POINTER(C.c_int32)), dp(weight), *[dp(a) if k in which else None for k, a in enumerate(out)])
    return rc, out


def test_same_bytes_twice_each_output_alone_another_seed_the_first_draws_and_another_handle():
    X, posterior = _case(70, N=300, n=40)
    ds, draws = _handle(X, posterior)
    lab = np.random.default_rng(71).integers(-1, 4, 300)
    w = np.random.default_rng(72).uniform(0.1, 2.0, 300)
    T = 4
    rc, a = _abi(ds, draws, lab, 4, T, w, seed=1)
    assert rc == 0 and all(not (x == -7.0).any() for x in a)
    rc, b = _abi(ds, draws, lab, 4, T, w, seed=1)
    assert rc == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for k in range(7):
        rc, alone = _abi(ds, draws, lab, 4, T, w, seed=1, which=[k])
        assert rc == 0 and alone[k].tobytes() == a[k].tobytes() and all((alone[j] == -7.0).all() for j in range(7) if j != k), NAMES[k]
    rc, other = _abi(ds, draws, lab, 4, T, w, seed=2)
    assert rc == 0 and all(other[k].tobytes() == a[k].tobytes() for k in range(4))            # another seed changes the path only
    assert all(not np.array_equal(other[k], a[k]) for k in range(4, 7))
    rc, few = _abi(ds, np.ascontiguousarray(draws[:7]), lab, 4, T, w, seed=1)
    assert rc == 0 and all(few[k].tobytes() == a[k][:7].tobytes() for k in range(7))
    # the engine's method: the same arrays, and only those asked for
    m = ds.trajectory_totals(draws, lab, 4, T, weight=w, seed=1)
    assert list(m) == list(NAMES) and all(m[k].tobytes() == x.tobytes() for k, x in zip(NAMES, a))
    some = ds.trajectory_totals(draws, lab, 4, T, weight=w, seed=1, outputs=("z", "equilibrium"))
    assert list(some) == ["equilibrium", "z"] and some["z"].tobytes() == a[4].tobytes()
    # a region without a site is 0
    rc, gap = _abi(ds, draws, np.where(lab == 2, -1, lab), 4, T, w, seed=1)
    assert rc == 0 and all(not x[..., 2].any() for x in gap) and all(x[..., 3].tobytes() == y[..., 3].tobytes() for x, y in zip(gap, a))
    # T = 1: the per-pair outputs are empty; asked for alone, there is nothing to do
    rc, single = _abi(ds, draws, lab, 4, 1, w, seed=1)
    assert rc == 0 and single[0].tobytes() == a[0][:, :1].tobytes() and single[1].shape == (40, 0, 4)
    rc, _ = _abi(ds, draws, lab, 4, 1, w, seed=1, which=[1, 2, 5, 6])
    assert rc == 0
    ds.close()
    # T is the call's: a handle of the same sites with 3 x 2 visits, observed ones among them, returns the same bytes
    Y = f32(np.random.default_rng(73).random((1, 300, 3, 2)) < 0.3)
    Y[0, ::5] = np.nan
    ds, _ = _handle(X, posterior, T=3, J=2, obs=Y)
    rc, c = _abi(ds, draws, lab, 4, T, w, seed=1)
    assert rc == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a, c))
    ds.close()


# ------------------------------------------------------------------------------------------ the forecast; obs_covs ----
def test_the_forecast_extends_the_expected_rows_and_redraws_the_path():
    X, posterior = _case(80, N=200, n=5)
    lab = np.random.default_rng(81).integers(0, 3, 200)
    w = np.random.default_rng(82).uniform(0.5, 2.0, 200)
    T = 4
    short = _compare(X, posterior, T, regions=lab, weights=w, seed=3, label="T")
    long = _compare(X, posterior, T + 3, regions=lab, weights=w, seed=3, label="T + 3")
    assert np.ascontiguousarray(long["occupancy"]["draws"][:, :T]).tobytes() == short["occupancy"]["draws"].tobytes()
    for k in ("colonised", "extinct", "growth_rate", "turnover"):
        assert np.ascontiguousarray(long[k]["draws"][:, :T - 1]).tobytes() == short[k]["draws"].tobytes(), k
    assert long["equilibrium"]["draws"].tobytes() == short["equilibrium"]["draws"].tobytes()
    # the path's cell index holds T: the first T seasons of the longer call are another draw of the same distribution
    assert not np.array_equal(long["z"]["draws"][:, :T], short["z"]["draws"])


def test_obs_covs_give_the_periods_and_nothing_else():
    X, posterior = _case(90, N=100)
    W = f32(np.random.default_rng(91).normal(size=(100, 4, 2, 1)))
    Y = f32(np.random.default_rng(92).random((1, 100, 4, 2)) < 0.3)
    lab = np.arange(100) % 3
    a = trajectory_totals(models.occu_dyn, posterior, site_covs=X, obs_covs=W, obs=Y, regions=lab, probs=PROBS, random_seed=4)
    b = trajectory_totals(models.occu_dyn, posterior, site_covs=X, n_periods=4, regions=lab, probs=PROBS, random_seed=4)
    assert a["n_periods"] == b["n_periods"] == 4
    for k in NAMES + ("growth_rate", "turnover"):
        assert all(a[k][s].tobytes() == b[k][s].tobytes() for s in ("draws", "mean", "sd", "quantiles")), k
    ref.check(a, X, posterior.sites, 4, lab, None, PROBS, 4, True, "obs_covs")
    c = trajectory_totals(models.occu_dyn, posterior, site_covs=X, obs_covs=W, n_periods=6, regions=lab, probs=PROBS, latent=False)
    assert c["n_periods"] == 6 and "z" not in c and c["occupancy"]["draws"].shape == (3, 6, 3, 1)
    ref.check(c, X, posterior.sites, 6, lab, None, PROBS, 0, False, "n_periods over obs_covs")


def test_the_first_season_is_the_host_paths_psi():
    """predict()'s psi is float32: (Ks + 4) 2^-24 relative per term stays below 1e-5 for Ks <= 8."""
    X, posterior = _case(95, N=150, Ks=8)
    W = np.zeros((150, 2, 1, 1), dtype=np.float32)
    w = np.random.default_rng(96).uniform(-1.0, 3.0, 150)
    preds = predict(models.occu_dyn, posterior, site_covs=X, obs_covs=W, num_samples=3)
    got = trajectory_totals(models.occu_dyn, posterior, site_covs=X, obs_covs=W, weights=w)
    want = (w * np.asarray(preds["psi"], dtype=np.float64)[:, :, 0]).sum(axis=1)
    assert np.all(np.abs(got["occupancy"]["draws"][:, 0, 0, 0] - want) <= 1e-5 * np.abs(w).sum())


# ------------------------------------------------------------------------------------------ a real fit ----
def test_a_small_fit():
    with contextlib.redirect_stdout(io.StringIO()):
        data, _ = simulate_dyn(n_sites=60, n_periods=4, random_seed=1)
    res = fit(models.occu_dyn, **data, num_chains=1, num_samples=100, num_warmup=100, timeout=600)
    rng = np.random.default_rng(97)
    N = 500
    grid = f32(rng.normal(size=(N, np.shape(data["site_covs"])[1])))
    lab = np.array(["north", "south", "east", "west"])[rng.integers(0, 4, N)]
    area = rng.uniform(0.5, 2.0, N)
    got = trajectory_totals(models.occu_dyn, res.mcmc, site_covs=grid, n_periods=7, regions=lab, weights=area, random_seed=7)
    assert got["n_draws"] == 100 and got["n_periods"] == 7 and list(got["regions"]) == ["east", "north", "south", "west"]
    ref.check(got, grid, res.mcmc.get_samples(), 7, lab, area, (0.05, 0.5, 0.95), 7, True, "fit")
    for k in NAMES + ("growth_rate", "turnover"):
        assert all(np.isfinite(got[k][s]).all() for s in ("draws", "mean", "sd", "quantiles")), k
        q = got[k]["quantiles"]
        assert np.all(q[0] <= q[1]) and np.all(q[1] <= q[2]) and np.all(q >= 0), k
    for k in NAMES:
        assert np.all(got[k]["draws"] <= got["weight"][:, None]), k
    # the fitted sites themselves, seasons from the data
    own = trajectory_totals(models.occu_dyn, res.mcmc, **data)
    assert own["n_periods"] == 4 and own["occupancy"]["draws"].shape == (100, 4, 1, 1) and np.all(own["occupancy"]["draws"] <= 60)


# ------------------------------------------------------------------------------------------ the C-ABI's refusals ----
def test_refusals_at_the_abi():
    rng = np.random.default_rng(0)
    X, W = f32(rng.normal(size=(20, 1))), f32(rng.normal(size=(20, 2, 2, 1)))
    Y = f32(rng.random((1, 20, 2, 2)) < 0.4)
    lab = np.arange(20) % 3
    untouched = lambda out: all((x == -7.0).all() for x in out)
    for name, opts in (("occu", {}), ("occu_rn", {}), ("nmixture", dict(max_abundance=3))):
        ds = OccuDataset(X, W, Y, model=name, **opts)
        dr = np.zeros((2, ds.D), dtype=np.float32)
        rc, out = _abi(ds, dr, lab, 3, 2)
        assert rc == _ffi.BL_ERR_UNSUPPORTED and b"bl_trajectory_totals: not built for " + name.encode() in ds._lib.bl_last_error(), name
        assert untouched(out), name
        with pytest.raises(NotImplementedError):
            ds.trajectory_totals(dr, lab, 3, 2)
        ds.close()
    ds = OccuDataset(X, W, Y, model="occu_dyn")
    dr = np.zeros((3, ds.D), dtype=np.float32)
    last = ds._lib.bl_last_error
    for T in (0, -1):
        rc, out = _abi(ds, dr, lab, 3, T)
        assert rc == _ffi.BL_ERR_INVALID and b"n_periods=%d" % T in last() and untouched(out), T
    for bad, G in ((3, 3), (-2, 3)):   # label G, label -2
        rc, out = _abi(ds, dr, np.where(np.arange(20) == 11, bad, lab), G, 2)
        assert rc == _ffi.BL_ERR_INVALID and b"bl_trajectory_totals: region[11]=%d outside -1 .. n_regions - 1 = 2" % bad in last(), bad
        assert untouched(out), bad
    w = np.ones(20)
    for bad in (np.nan, np.inf):
        w[4] = bad
        rc, out = _abi(ds, dr, lab, 3, 2, w)
        assert rc == _ffi.BL_ERR_INVALID and b"weight[4]=" + str(bad).encode() in last() and untouched(out), bad
    rc, out = _abi(ds, dr, lab, 3, 2, which=())                # every output NULL
    assert rc == _ffi.BL_ERR_INVALID and untouched(out)
    rc, out = _abi(ds, dr, np.full(20, -1), 0, 2)              # n_regions = 0
    assert rc == _ffi.BL_ERR_INVALID and b"n_regions=0" in last() and untouched(out)
    with pytest.raises(ValueError):
        ds.trajectory_totals(dr, lab[:5], 3, 2)
    with pytest.raises(ValueError):
        ds.trajectory_totals(dr, lab, 3, 2, outputs=())
    with pytest.raises(ValueError):
        ds.trajectory_totals(dr, lab, 3, 2, outputs=("psi",))
    with pytest.raises(ValueError):
        ds.trajectory_totals(dr, lab, 3, 0)
    # every site in no region: the totals are zeros
    rc, out = _abi(ds, dr, np.full(20, -1), 2, 2)
    assert rc == 0 and all(not x.any() for x in out)
    # a NUTS launch in flight
    ds.launch(num_warmup=200000, num_samples=200000, num_chains=2, seed=0)
    rc, out = _abi(ds, dr, lab, 3, 2)
    assert rc == _ffi.BL_ERR_BUSY and b"in flight" in last() and untouched(out)
    ds.abort()
    with pytest.raises(Exception, match="aborted"):
        ds.wait()
    rc, out = _abi(ds, dr, lab, 3, 2)
    assert rc == 0 and not any((x == -7.0).any() for x in out)   # the handle stays usable
    ds.close()
