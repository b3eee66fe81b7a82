"""site_diagnostics on the GPU: the fused effective sample size and split R-hat (bl_site_diagnostics) of the two deterministic sites
against their definition in NumPy on predict()'s arrays (tests/diagnostics_ref.py: direct lagged sums in float64) for every served
handle; two species; the geometry (one site, a tail block, one period and one replicate, no covariates, sixteen per side, and every
covariate count the kernels are instantiated for); 1 x 2, 1 x 5, 2 x 3, 4 x 17, 3 x 65 and 4 x 257 chains x draws; AR(1) coefficients 0,
0.9 and -0.6; chains with offset means (every pair of Geyer's sequence live); draws that are all equal (NaN); saturated values (exact
0.0f and 1.0f, rates of 1e36); mean and sd bit-equal to site_summary's; the same bytes twice, from each output alone and from a data set
of the first sites alone; the refusals at the C-ABI; a small real fit against bench.ess_of_site_function.

Posteriors are hand-made behind a ``get_samples()`` / ``num_chains`` stub: every coefficient's draws are an AR(1) series along the draw
axis, chain by chain, so the value series are autocorrelated.  The bounds are tests/diagnostics_ref.py's; they are derived there, not
tuned.  occu_cs: predict() returns ``psi`` only, so its second site is compared with the engine's ``deterministic`` -- the kernel behind
predict()'s ``prob_detection``.

The kernels sum BL_SD_LAGS = 32 lags (16 pairs) a pass over the chains: 4 x 257 with offset chain means has 128 live pairs and takes all
eight passes, 3 x 65 two, 4 x 17 one."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest

import diagnostics_ref
from biolith_amd import _ffi, models
from biolith_amd.engine import OccuDataset
from biolith_amd.models import simulate
from biolith_amd.utils import fit, predict, site_diagnostics, site_summary
from biolith_amd.utils.data import prepare_data, species_dataset
from biolith_amd.utils.layout import draws_from_sites, layout_for
from biolith_amd.utils.site_summary import site_names

pytestmark = pytest.mark.gpu

KEYS = ("n_eff", "r_hat", "mean", "sd")
f32 = lambda a: np.asarray(a, dtype=np.float32)


class _Posterior:
    """What predict and site_diagnostics read of a fit: ``get_samples()`` and ``num_chains``."""

    def __init__(self, sites, num_chains):
        self.sites, self.num_chains = sites, num_chains

    def get_samples(self):
        return self.sites


def _ar1(rng, chains, n, shape, phi, sd=1.0, lo=None):
    """(chains n,) + shape, chain-major: per chain a stationary AR(1) series of standard deviation ``sd`` along the draws."""
    z = np.empty((chains, n) + tuple(shape))
    e = rng.normal(size=z.shape)
    z[:, 0] = e[:, 0]
    for t in range(1, n):
        z[:, t] = phi * z[:, t - 1] + np.sqrt(1.0 - phi * phi) * e[:, t]
    z = sd * z.reshape((chains * n,) + tuple(shape))
    return z if lo is None else lo + np.abs(z)


def _case(name, seed, N=37, T=2, J=3, chains=2, n=33, Ks=2, Ko=2, S=1, fp=None, site_re=False, obs_re=False, scale=0.6, phi=0.9, offset=0.0):
    """Random covariates, a hand-made autocorrelated posterior of ``chains`` x ``n`` draws for them, and the model's options.  ``offset``
    moves chain c's intercepts by ``c * offset``."""
    rng = np.random.default_rng(seed)
    data = dict(site_covs=f32(rng.normal(size=(N, Ks))), obs_covs=f32(rng.normal(size=(N, T, J, Ko))))
    ar = lambda shape=(), sd=scale, lo=None: _ar1(rng, chains, n, shape, phi, sd, lo)
    sites = dict(beta=ar((S, Ks + 1)), alpha=ar((S, Ko + 1)))
    shift = offset * np.repeat(np.arange(chains), n)
    sites["beta"][:, :, 0] += shift[:, None]
    sites["alpha"][:, :, 0] -= shift[:, None]
    opts = {}
    if name == "occu_cop":
        opts["session_duration"] = f32(rng.uniform(0.5, 9.0, (N, T, J)))
    if name == "occu_cs":
        mu0 = ar(sd=1.0)
        sites.update(mu0=mu0, mu1=mu0 + ar(sd=1.0, lo=0.5), sigma0=ar(sd=0.5, lo=0.5), sigma1=ar(sd=0.5, lo=0.5))
    if fp:
        opts[f"false_positives_{fp}"] = True
        sites[f"prob_fp_{fp}"] = np.clip(ar(sd=0.1, lo=0.05), 0.05, 0.6)
    if site_re:
        opts["site_random_effects"] = True
        first = "site_re_abu" if name in ("occu_rn", "nmixture") else "site_re_occ"
        sites.update({"site_re_sd": ar(sd=0.3, lo=0.3), first: ar((N, S), sd=0.5), "site_re_det": ar((N, S), sd=0.5)})
    if obs_re:
        opts["obs_random_effects"] = True
        sites.update(obs_re_sd=ar(sd=0.3, lo=0.3), obs_re=ar((J, T, N, S), sd=0.5))
    return data, _Posterior({k: f32(v) for k, v in sites.items()}, chains), opts


def _handle(name, data, posterior, opts, sp=0):
    """Species ``sp``'s handle and draw matrix, made as predict() and site_diagnostics make them."""
    site_covs, obs_covs, _, dur, _, _ = prepare_data(data["site_covs"], data["obs_covs"], None, opts.get("session_duration"))
    S = posterior.sites["beta"].shape[1]
    rest = {k: v for k, v in opts.items() if k != "session_duration"}
    valid = {k: v for k, v in dict(site_covs=site_covs, obs_covs=obs_covs, session_duration=dur).items() if v is not None}
    spec = getattr(models, name)(**valid, obs=np.full((S,) + np.shape(obs_covs)[:3], np.nan, dtype=np.float32), **rest)
    N, T, J, Ko = spec.obs_covs.shape
    layout = layout_for(spec, N=N, T=T, J=J, Ks=spec.site_covs.shape[1], Ko=Ko)
    return species_dataset(spec, sp, 0), draws_from_sites(layout, posterior.sites, sp)


def _compare(name, data, posterior, opts, label=""):
    """The wrapper against the definition on predict()'s arrays; mean and sd bit-equal to site_summary's.  Returns the wrapper's result,
    the definition's per site and predict()'s two arrays (occu_cs: the second from ``deterministic``)."""
    model = getattr(models, name)
    total, S = posterior.sites["beta"].shape[:2]
    chains = posterior.num_chains
    preds = predict(model, posterior, **data, num_samples=total, **opts)
    got = site_diagnostics(model, posterior, **data, **opts)
    summary = site_summary(model, posterior, **data, probs=[0.5], **opts)
    first, second = site_names(name)
    assert set(got) == {first, second, "n_chains", "n_draws"} and got["n_chains"] == chains and got["n_draws"] == total // chains
    v1, v2 = f32(preds[first]), []
    assert np.array_equal(v1, np.broadcast_to(v1[:, :1], v1.shape))   # constant over the periods, as the entry returns it
    for sp in range(S):
        if name == "occu_cs":
            ds, draws = _handle(name, data, posterior, opts, sp)
            v2.append(ds.deterministic(draws, psi=False, prob_detection=True)[1].copy())
            ds.close()
        else:
            v2.append(f32(preds[second])[..., sp])
    v2 = np.stack(v2, axis=-1)
    want = {}
    for site, v in ((first, v1), (second, v2)):
        want[site] = diagnostics_ref.check(got[site], v, chains, f"{label} {site}")
        for k in ("mean", "sd"):
            assert got[site][k].tobytes() == summary[site][k].tobytes(), f"{label}: {site} {k} is not site_summary's"
    return got, want, v1, v2


# ------------------------------------------------------------------------------------------ every served handle ----
HANDLES = [("occu", {}), ("occu", dict(fp="constant")), ("occu", dict(fp="unoccupied")), ("occu", dict(site_re=True)),
           ("occu", dict(obs_re=True)), ("occu", dict(site_re=True, obs_re=True)), ("occu_rn", {}), ("nmixture", {}), ("occu_cop", {}),
           ("occu_cs", {})]


@pytest.mark.parametrize("name,options", HANDLES, ids=[h[0] + "".join("-" + k + ("_" + v if isinstance(v, str) else "") for k, v in h[1].items())
                                                       for h in HANDLES])
def test_every_served_handle(name, options):
    _compare(name, *_case(name, 1, **options), label=f"{name} {options}")


def test_two_species():
    data, posterior, opts = _case("occu", 2, S=2)
    both, _, _, _ = _compare("occu", data, posterior, opts, label="S=2")
    assert both["psi"]["n_eff"].shape == (2, 37, 2) and both["prob_detection"]["r_hat"].shape == (3, 2, 37, 2)
    # the species are handled in a loop: species 1 alone is its part of the plate, bit for bit
    one = site_diagnostics(models.occu, _Posterior({k: v[:, 1:] for k, v in posterior.sites.items()}, 2), **data)
    for site in ("psi", "prob_detection"):
        for k in KEYS + ("mcse_mean",):
            assert one[site][k].tobytes() == np.ascontiguousarray(both[site][k][..., 1:]).tobytes(), (site, k)


# ------------------------------------------------------------------------------------------ geometry ----
# (the kernels are instantiated for 0 .. 4 covariates on the cell's side and once for any number: each form on either side)
@pytest.mark.parametrize("shape", [dict(N=1), dict(N=257), dict(T=1, J=1), dict(Ks=0, Ko=0), dict(Ks=16, Ko=16, scale=0.3), dict(Ks=1, Ko=4),
                                   dict(Ks=4, Ko=1), dict(Ks=3, Ko=3), dict(Ks=5, Ko=5)],
                         ids=["one_site", "a_tail_block", "one_period_one_replicate", "intercepts_only", "sixteen_covariates", "Ks1_Ko4", "Ks4_Ko1",
                              "Ks3_Ko3", "Ks5_Ko5"])
def test_geometry(shape):
    got, _, v1, _ = _compare("occu", *_case("occu", 3, n=20, **shape), label=str(shape))
    if shape.get("Ks") == 0:   # every site is the same series
        assert np.all(got["psi"]["n_eff"] == got["psi"]["n_eff"][:1, :1]) and np.all(v1 == v1[:, :1, :1])


# ------------------------------------------------------------------------------------------ chains x draws, series ----
@pytest.mark.parametrize("chains,n", [(1, 2), (1, 5), (2, 3), (4, 17), (3, 65), (4, 257)])
def test_chains_and_draws(chains, n):
    """With offset chain means (more than one chain) every pair stays live: the wave takes every pass over the lags, BL_SD_LAGS = 32
    (biolith_amd/csrc/site_diagnostics.hpp) a pass -- one for 17 draws, two for 65, eight for 257, the last one short."""
    data, posterior, opts = _case("occu", 4, chains=chains, n=n, offset=3.0 if chains > 1 else 0.0)
    got, want, v1, v2 = _compare("occu", data, posterior, opts, label=f"{chains} x {n}")
    if n < 4:
        assert np.isnan(got["psi"]["r_hat"]).all() and np.isnan(got["prob_detection"]["r_hat"]).all()   # a half of one draw
    if chains > 1 and n >= 4:
        _, info = diagnostics_ref.reference(v1, chains)
        assert info["live"].max() == n // 2 and (got["psi"]["r_hat"] > 1.0).all()


@pytest.mark.parametrize("offset", [0.0, 3.0], ids=["mixed", "offset_chain_means"])
@pytest.mark.parametrize("phi", [0.0, 0.9, -0.6])
def test_series(phi, offset):
    data, posterior, opts = _case("occu", 5, chains=4, n=65, phi=phi, offset=offset)
    _, _, v1, _ = _compare("occu", data, posterior, opts, label=f"phi={phi} offset={offset}")
    live = diagnostics_ref.reference(v1, 4)[1]["live"]
    if offset:
        assert live.max() == 32
    elif phi <= 0:
        assert live.max() < 16   # (stops within the first pass)


def test_draws_that_are_all_equal_give_nan():
    data, posterior, opts = _case("occu", 6, chains=2, n=9)
    same = _Posterior({k: np.repeat(v[:1], 18, axis=0) for k, v in posterior.sites.items()}, 2)
    got, _, v1, v2 = _compare("occu", data, same, opts, label="all equal")
    for site, v in (("psi", v1), ("prob_detection", v2)):
        assert np.isnan(got[site]["n_eff"]).all() and np.isnan(got[site]["r_hat"]).all() and np.isnan(got[site]["mcse_mean"]).all()
        assert np.array_equal(got[site]["mean"], v[0].astype(np.float64)) and not got[site]["sd"].any()
    # one site constant, the other not: psi's draws are equal, the detection coefficients move
    mixed = _Posterior(dict(beta=same.sites["beta"], alpha=posterior.sites["alpha"]), 2)
    got, _, _, _ = _compare("occu", data, mixed, opts, label="psi equal")
    assert np.isnan(got["psi"]["n_eff"]).all() and np.isfinite(got["prob_detection"]["n_eff"]).all()


# ------------------------------------------------------------------------------------------ saturation ----
def test_saturated_probabilities():
    data, posterior, opts = _case("occu", 7, chains=2, n=32)
    for site in ("beta", "alpha"):
        for first in (0, 32):
            posterior.sites[site][first:first + 10, :, 0] = 100.0        # 1.0f exactly
            posterior.sites[site][first + 10:first + 22, :, 0] = -100.0  # 0.0f exactly
    _, _, v1, v2 = _compare("occu", data, posterior, opts, label="saturated")
    for v in (v1, v2):
        assert (v == 1.0).any() and (v == 0.0).any() and ((v > 0.0) & (v < 1.0)).any()


def test_saturated_rates():
    data, posterior, opts = _case("occu_rn", 8, chains=2, n=32, scale=0.3)
    posterior.sites["beta"][:, 0, 0] = f32(np.tile(np.linspace(-20.0, 83.0, 32), 2))
    _, _, v1, _ = _compare("occu_rn", data, posterior, opts, label="rates")
    assert np.isfinite(v1).all() and v1.max() > 1e36 and v1.min() < 1e-6


# ------------------------------------------------------------------------------------------ determinism ----
def _abi(ds, draws, chains, which=range(8)):
    """bl_site_diagnostics through ctypes with only the outputs ``which`` (0 .. 7 in the entry's order) passed; the others stay untouched."""
    shapes = [(ds.N,)] * 4 + [(ds.J, ds.T, ds.N)] * 4
    out = [np.full(s, -7.0) for s in shapes]
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = ds._lib.bl_site_diagnostics(ds._h, draws.shape[0], draws.ctypes.data_as(C.POINTER(C.c_float)), chains,
                                     *[ptr(a) if k in which else None for k, a in enumerate(out)])
    return rc, out


def test_same_bytes_twice_and_each_output_alone():
    data, posterior, opts = _case("occu", 9, N=300, chains=2, n=40, offset=3.0)
    ds, draws = _handle("occu", data, posterior, opts)
    rc, a = _abi(ds, draws, 2)
    assert rc == 0 and all(not (x == -7.0).any() for x in a)
    rc, b = _abi(ds, draws, 2)
    assert rc == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for k in range(8):
        rc, alone = _abi(ds, draws, 2, which=[k])
        assert rc == 0 and alone[k].tobytes() == a[k].tobytes(), k
        assert all((x == -7.0).all() for j, x in enumerate(alone) if j != k), k
    # the engine's method: the same arrays, None where not wanted
    m = ds.site_diagnostics(draws, 2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(m, a))
    assert [x is None for x in ds.site_diagnostics(draws, 2, psi=False)] == [True] * 4 + [False] * 4
    assert [x is None for x in ds.site_diagnostics(draws, 2, prob_detection=False)] == [False] * 4 + [True] * 4
    # the chain count is part of the definition: other chains, other numbers (the mean and sd over all draws stay)
    other = ds.site_diagnostics(draws, 4)
    assert other[0].tobytes() != a[0].tobytes() and other[2].tobytes() == a[2].tobytes() and other[3].tobytes() == a[3].tobytes()
    ds.close()


def test_the_first_sites_alone_give_the_same_bytes():
    data, posterior, opts = _case("occu", 10, N=300, chains=2, n=40)
    ds, draws = _handle("occu", data, posterior, opts)
    few = OccuDataset(data["site_covs"][:5], data["obs_covs"][:5], np.full((1, 5, 2, 3), np.nan, dtype=np.float32))
    whole, part = ds.site_diagnostics(draws, 2), few.site_diagnostics(draws, 2)
    for k, (a, b) in enumerate(zip(whole, part)):
        assert np.ascontiguousarray(a[..., :5]).tobytes() == b.tobytes(), k
    ds.close(); few.close()


# ------------------------------------------------------------------------------------------ the C-ABI's refusals ----
def test_refusals_at_the_abi():
    rng = np.random.default_rng(0)
    X, W = f32(rng.normal(size=(20, 1))), f32(rng.normal(size=(20, 2, 2, 1)))
    Y = f32(rng.random((1, 20, 2, 2)) < 0.4)
    blank = lambda J: np.full((1, 20, 2, J), np.nan, dtype=np.float32)
    refused = {"joint-species": (OccuDataset(X, W, np.concatenate([Y, Y])), b"bl_site_diagnostics: a joint-species handle"),
               "occu_dyn": (OccuDataset(X, W, Y, model="occu_dyn"), b"bl_site_diagnostics: the dynamic occupancy model's sites"),
               "occu_comb": (OccuDataset(X, W, blank(2), model="occu_comb", ARU_obs_covs=rng.normal(size=(20, 2, 3, 1)), ARU_obs=blank(3),
                                         scores_obs=blank(2)),
                             b"bl_site_diagnostics: occu_comb's sites")}
    for name, (ds, message) in refused.items():
        dr = np.zeros((4, ds.D), dtype=np.float32)
        rc, out = _abi(ds, dr, 2)
        assert rc == _ffi.BL_ERR_UNSUPPORTED and message in ds._lib.bl_last_error(), name
        assert all((x == -7.0).all() for x in out), name
        with pytest.raises(NotImplementedError):
            ds.site_diagnostics(dr, 2)
        ds.close()
    ds = OccuDataset(X, W, Y)
    dr = np.zeros((6, ds.D), dtype=np.float32)
    last = ds._lib.bl_last_error
    for chains, message in ((4, b"n_draws=6 is not n_chains=4 chains of equal length"), (0, b"n_chains=0"), (-1, b"n_chains=-1"),
                            (6, b"1 draws per chain, at least 2"), (5, b"n_chains=5")):
        rc, out = _abi(ds, dr, chains)
        assert rc == _ffi.BL_ERR_INVALID and message in last(), chains
        assert all((x == -7.0).all() for x in out), chains
    rc, _ = _abi(ds, dr, 2, which=[])                                                          # every output NULL
    assert rc == _ffi.BL_ERR_INVALID
    assert ds._lib.bl_site_diagnostics(ds._h, 0, dr.ctypes.data_as(C.POINTER(C.c_float)), 1, *([None] * 8)) == _ffi.BL_ERR_INVALID
    assert _abi(ds, dr, 3)[0] == 0                                                             # 3 x 2: the shortest chains pass
    with pytest.raises(ValueError):
        ds.site_diagnostics(dr, 4)
    with pytest.raises(ValueError):
        ds.site_diagnostics(dr, 6)
    with pytest.raises(ValueError):
        ds.site_diagnostics(dr, 2, psi=False, prob_detection=False)
    ds.close()


# ------------------------------------------------------------------------------------------ a real fit ----
def test_a_small_fit():
    """60 sites, 2 chains x 100 draws: against the definition on predict()'s arrays, and mean(n_eff of psi) against
    bench.ess_of_site_function -- the host's FFT estimator on psi formed in float64 and rounded to float32, which is not the device's
    float32 value bit for bit.  Its distance: the predictor's |eta| 2^-24 through exp, three roundings of the quotient, one of the
    host's -- below 8 2^-24 in psi for |eta| <= 16 (tests/diagnostics_ref.py carries it through: ``eps``).  Carried through as a
    worst case that distance gives about a tenth of n_eff: this last assertion is a SANITY CHECK of the interface -- the chain
    order, the site, the mean over the sites are bench.py's -- and shows nothing about precision; the ``check`` calls above do.
    A fit's ``get_samples()`` holds the deterministic sites as lazy thunks: the call must not fire them."""
    import bench

    with contextlib.redirect_stdout(io.StringIO()):
        data, _ = simulate(n_sites=60, random_seed=1)
    res = fit(models.occu, **data, num_chains=2, num_samples=100, num_warmup=100, timeout=600)

    class _Untouched:
        """The fit's mcmc with every lazy site's thunk replaced by one that fails the test."""
        num_chains = res.mcmc.num_chains

        def get_samples(self):
            def thunk():
                raise AssertionError("a lazy deterministic site was materialised")

            samples = res.mcmc.get_samples()
            assert {"psi", "prob_detection"} <= set(samples._lazy)
            for k in list(samples._lazy):
                samples.set_lazy(k, thunk)
            return samples

    got = site_diagnostics(models.occu, res.mcmc, **data)
    lazy = site_diagnostics(models.occu, _Untouched(), **data)
    assert all(lazy[site][k].tobytes() == got[site][k].tobytes() for site in ("psi", "prob_detection") for k in KEYS)
    preds = predict(models.occu, res.mcmc, **data, num_samples=200)
    assert got["n_chains"] == 2 and got["n_draws"] == 100
    for site in ("psi", "prob_detection"):
        diagnostics_ref.check(got[site], f32(preds[site]), 2, f"fit {site}")
        assert np.all(got[site]["n_eff"] > 1) and np.all(got[site]["r_hat"] > 0.9) and np.all(got[site]["mcse_mean"] < got[site]["sd"])
    only = site_diagnostics(models.occu, res.mcmc, **data, sites=["psi"])
    assert "prob_detection" not in only and only["psi"]["n_eff"].tobytes() == got["psi"]["n_eff"].tobytes()
    one_chain = site_diagnostics(models.occu, res.mcmc, **data, sites="psi", num_chains=1)   # the keyword overrides mcmc.num_chains
    assert one_chain["n_chains"] == 1 and one_chain["n_draws"] == 200
    diagnostics_ref.check(one_chain["psi"], f32(preds["psi"]), 1, "fit psi as one chain")
    # the headline figure, as bench.py computes it
    X = np.asarray(prepare_data(data["site_covs"], data["obs_covs"], None, None)[0], dtype=np.float64)
    draws = np.asarray(res.mcmc.result.draws, dtype=np.float64)
    assert np.abs(draws[..., :1] + draws[..., 1:X.shape[1] + 1] @ X.T).max() <= 16.0
    host = bench.ess_of_site_function(draws, X, "psi")
    _, bound = diagnostics_ref.reference(f32(preds["psi"])[:, 0, :, 0], 2, eps=8 * 2.0 ** -24)
    mine = float(np.mean(got["psi"]["n_eff"][0, :, 0]))
    print(f"mean n_eff of psi: fused {mine:.6f}  bench {host:.6f}  |difference| {abs(mine - host):.3e}  bound {float(np.mean(bound['n_eff'])):.3e}")
    assert np.isfinite(bound["n_eff"]).all() and abs(mine - host) <= float(np.mean(bound["n_eff"]))
