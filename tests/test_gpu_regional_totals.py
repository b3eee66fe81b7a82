"""regional_totals on the GPU: the fused totals (bl_regional_totals) against their definition in NumPy on predict()'s arrays for the
same seed (tests/totals_ref.py) for every served model and handle kind; the geometry (one site, sizes around a wave and a block,
interleaved labels, a draw loop that strides past the grid rows, a chunk boundary); predict()'s values bit for bit where every site is
its own region; two species; the locality of a region's rows; zero, negative and unit weights; the same bytes twice, from each output
alone, under another seed and from the first draws; a small real fit; the refusals at the C-ABI.

Posteriors are hand-made (random float32 coefficients in (-1, 1) behind a ``get_samples()`` stub); one fit of 60 sites, 100 + 100
draws.  Both sides sum the same float64 terms, so the bound is derived (tests/totals_ref.py):
``|got - want| <= 2 (N_g - 1) 2^-53 sum_{i in g} |w_i v_i|``; with unit weights the latent totals are integers: equality."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest

import totals_ref
from biolith_amd import _ffi, models
from biolith_amd.engine import OccuDataset
from biolith_amd.models import simulate
from biolith_amd.utils import fit, predict, regional_totals
from biolith_amd.utils.data import prepare_data, species_dataset
from biolith_amd.utils.layout import draws_from_sites, layout_for
from biolith_amd.utils.regional_totals import total_names

pytestmark = pytest.mark.gpu

PROBS = (0.05, 0.5, 0.95)
f32 = lambda a: np.asarray(a, dtype=np.float32)


class _Posterior:
    """What predict and regional_totals read of a fit: ``get_samples()``."""

    def __init__(self, sites):
        self.sites = sites

    def get_samples(self):
        return self.sites


def _case(name, seed, N=70, T=2, J=2, n=3, Ks=2, Ko=1, S=1, fp=None, site_re=False, obs_re=False, **more):
    """Random covariates, a hand-made posterior for them (coefficients in (-1, 1)), and the model's options."""
    rng = np.random.default_rng(seed)
    data = dict(site_covs=f32(rng.normal(size=(N, Ks))), obs_covs=f32(rng.normal(size=(N, T, J, Ko))))
    sites = dict(beta=f32(rng.uniform(-1, 1, (n, S, Ks + 1))), alpha=f32(rng.uniform(-1, 1, (n, S, Ko + 1))))
    opts = dict(more)
    if name == "occu_cop":
        opts["session_duration"] = f32(rng.uniform(0.5, 9.0, (N, T, J)))
    if name == "occu_cs":
        mu0 = rng.normal(0, 1, n)
        sites.update(mu0=f32(mu0), mu1=f32(mu0 + rng.uniform(0.5, 3.0, n)), sigma0=f32(rng.uniform(0.5, 2.0, n)), sigma1=f32(rng.uniform(0.5, 2.0, n)))
    if fp:
        opts[f"false_positives_{fp}"] = True
        sites["rate_fp_" + fp if name == "occu_cop" else "prob_fp_" + fp] = f32(rng.uniform(0.05, 0.3, n))
    if site_re:
        opts["site_random_effects"] = True
        first = "site_re_abu" if name in ("occu_rn", "nmixture") else "site_re_occ"
        sites.update({"site_re_sd": f32(rng.uniform(0.3, 1.0, n)), first: f32(rng.normal(0, 0.5, (n, N, S))),
                      "site_re_det": f32(rng.normal(0, 0.5, (n, N, S)))})
    if obs_re:
        opts["obs_random_effects"] = True
        sites.update(obs_re_sd=f32(rng.uniform(0.3, 1.0, n)), obs_re=f32(rng.normal(0, 0.5, (n, J, T, N, S))))
    return data, _Posterior(sites), opts


def _handle(name, data, posterior, opts, sp=0):
    """Species ``sp``'s handle and draw matrix, made as predict() and regional_totals make them."""
    site_covs, obs_covs, _, dur, _, _ = prepare_data(data["site_covs"], data["obs_covs"], None, opts.get("session_duration"))
    S = posterior.sites["beta"].shape[1]
    rest = {k: v for k, v in opts.items() if k != "session_duration"}
    valid = {k: v for k, v in dict(site_covs=site_covs, obs_covs=obs_covs, session_duration=dur).items() if v is not None}
    spec = getattr(models, name)(**valid, obs=np.full((S,) + np.shape(obs_covs)[:3], np.nan, dtype=np.float32), **rest)
    N, T, J, Ko = spec.obs_covs.shape
    layout = layout_for(spec, N=N, T=T, J=J, Ks=spec.site_covs.shape[1], Ko=Ko)
    return species_dataset(spec, sp, 0), draws_from_sites(layout, posterior.sites, sp)


def _compare(name, data, posterior, opts, regions=None, weights=None, seed=0, label=""):
    """The wrapper against the definition on predict()'s arrays for the same seed.  Returns the wrapper's result and predict()'s."""
    model = getattr(models, name)
    n = posterior.sites["beta"].shape[0]
    preds = predict(model, posterior, **data, num_samples=n, random_seed=seed, **opts)
    got = regional_totals(model, posterior, **data, regions=regions, weights=weights, probs=PROBS, random_seed=seed, **opts)
    first, second = total_names(name)
    worst = totals_ref.check(got, preds, first, second, regions, weights, PROBS, label)
    print(f"{label}: largest error {worst:.3g} of its bound")
    return got, preds


def _interleaved(N, seed=0):
    """Labels of N >= 256 sites in no order: regions of 1, 63, 64 and 65 sites and one of the remainder."""
    lab = np.repeat(np.array(["one", "w63", "w64", "w65", "rest"]), [1, 63, 64, 65, N - 193])
    return np.random.default_rng(seed).permutation(lab)


# ------------------------------------------------------------------------------------------ geometry ----
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 300])
@pytest.mark.parametrize("n", [1, 3])
def test_one_region(N, n):
    data, posterior, opts = _case("occu", N, N=N, n=n)
    w = np.random.default_rng(N).uniform(0.1, 5.0, N)
    got, _ = _compare("occu", data, posterior, opts, weights=w, label=f"N={N} n={n}")
    assert list(got["regions"]) == ["all"] and got["psi"]["draws"].shape == (n, 1, 1) and got["z"]["draws"].shape == (n, 2, 1, 1)
    if n == 1:
        assert np.isnan(got["psi"]["sd"]).all() and np.isnan(got["z"]["sd"]).all()


@pytest.mark.parametrize("n", [1, 3])
def test_interleaved_labels(n):
    data, posterior, opts = _case("occu", 11, N=300, n=n)
    lab = _interleaved(300)
    assert not np.array_equal(lab, np.sort(lab))
    w = np.random.default_rng(1).uniform(0.1, 5.0, 300)
    got, _ = _compare("occu", data, posterior, opts, regions=lab, weights=w, label=f"interleaved n={n}")
    assert list(got["regions"]) == ["one", "rest", "w63", "w64", "w65"] and list(got["n_sites"]) == [1, 107, 63, 64, 65]
    _compare("occu", data, posterior, opts, regions=lab, label=f"interleaved, unit weights n={n}")


def test_the_draw_loop_strides_past_the_grid_rows():
    data, posterior, opts = _case("occu", 12, N=40, n=1100)
    lab = np.random.default_rng(2).integers(0, 3, 40)
    _compare("occu", data, posterior, opts, regions=lab, weights=np.linspace(-1.0, 2.0, 40), label="n=1100")


def test_a_chunk_boundary():
    """One region per site at N = 11 000: 11 000 waves x 3 output rows x 8 bytes a draw, so 1016 draws fill the 256 MB of the workspace
    and the 1100 draws go through in two chunks.  Every total is one term: predict()'s value times the weight, bit for bit."""
    N, n = 11000, 1100
    data, posterior, opts = _case("occu", 13, N=N, n=n, J=1)
    ds, draws = _handle("occu", data, posterior, opts)
    w = np.random.default_rng(3).normal(size=N)
    site, lat = ds.regional_totals(draws, np.arange(N), N, weight=w, seed=5)
    psi = ds.deterministic(draws)[0]
    z = ds.predictive(draws, seed=5, y=False)[0]
    ds.close()
    assert site.tobytes() == (w[None, :] * psi[:, 0].astype(np.float64)).tobytes()
    assert lat.tobytes() == (w[None, None, :] * z.astype(np.float64)).tobytes()


# ------------------------------------------------------------------------------------------ every served model and handle kind ----
HANDLES = [("occu", {}), ("occu", dict(fp="constant")), ("occu", dict(site_re=True, obs_re=True)), ("occu_cs", {}), ("occu_cop", {}),
           ("occu_cop", dict(fp="unoccupied")), ("occu_rn", {}), ("occu_rn", dict(site_re=True)), ("nmixture", dict(max_abundance=3))]
IDS = [h[0] + "".join("-" + k + ("_" + str(v) if not isinstance(v, bool) else "") for k, v in h[1].items()) for h in HANDLES]


@pytest.mark.parametrize("name,options", HANDLES, ids=IDS)
def test_every_served_handle(name, options):
    data, posterior, opts = _case(name, 20, **options)
    rng = np.random.default_rng(21)
    lab, w = rng.integers(0, 3, 70), rng.uniform(-1.0, 4.0, 70)
    got, preds = _compare(name, data, posterior, opts, regions=lab, weights=w, seed=3, label=f"{name} {options}")
    first, second = total_names(name)
    assert got[first]["draws"].shape == (3, 3, 1) and got[first]["quantiles"].shape == (3, 3, 1) and got[first]["mean"].shape == (3, 1)
    assert got[second]["draws"].shape == (3, 2, 3, 1) and got[second]["quantiles"].shape == (3, 2, 3, 1) and got[second]["sd"].shape == (2, 3, 1)
    _compare(name, data, posterior, opts, regions=lab, seed=3, label=f"{name} {options}, unit weights")
    if name == "nmixture":   # the restricted Poisson reaches its cap
        assert np.asarray(preds["N_i"]).max() == 3
    if name == "occu_cop":
        assert "session_duration" in opts


@pytest.mark.parametrize("name,options", HANDLES, ids=IDS)
def test_predicts_values_bit_for_bit(name, options):
    """Every site its own region (G = N = 65), arbitrary weights: a total is one term."""
    data, posterior, opts = _case(name, 30, N=65, **options)
    w = np.random.default_rng(31).normal(size=65) * 3.0
    model = getattr(models, name)
    preds = predict(model, posterior, **data, num_samples=3, random_seed=9, **opts)
    got = regional_totals(model, posterior, **data, regions=np.arange(65), weights=w, random_seed=9, **opts)
    first, second = total_names(name)
    v, z = f32(preds[first]), np.asarray(preds[second])
    assert got[first]["draws"].tobytes() == (w[None, :, None] * v[:, 0].astype(np.float64)).tobytes()
    assert got[second]["draws"].tobytes() == (w[None, None, :, None] * z.astype(np.float64)).tobytes()
    assert list(got["n_sites"]) == [1] * 65 and np.array_equal(got["weight"], w)


def test_two_species():
    data, posterior, opts = _case("occu", 40, S=2)
    lab = np.random.default_rng(41).integers(0, 3, 70)
    w = np.random.default_rng(42).uniform(0.5, 2.0, 70)
    both, _ = _compare("occu", data, posterior, opts, regions=lab, weights=w, seed=4, label="S=2")
    assert both["psi"]["draws"].shape == (3, 3, 2) and both["z"]["draws"].shape == (3, 2, 3, 2)   # the plate is last
    one = regional_totals(models.occu, _Posterior({k: v[:, :1] for k, v in posterior.sites.items()}), **data, regions=lab, weights=w,
                          probs=PROBS, random_seed=4)
    for site in ("psi", "z"):
        for k in ("draws", "mean", "sd", "quantiles"):
            assert one[site][k].tobytes() == np.ascontiguousarray(both[site][k][..., :1]).tobytes(), (site, k)


# ------------------------------------------------------------------------------------------ locality ----
def test_a_regions_rows_do_not_depend_on_the_other_sites_labels():
    N = 300
    data, posterior, opts = _case("occu_rn", 50, N=N, n=3)
    rng = np.random.default_rng(51)
    w = rng.uniform(-1.0, 3.0, N)
    in_a = rng.random(N) < 0.4
    others = np.flatnonzero(~in_a)
    one = np.where(in_a, "A", "B")
    three = one.copy()
    three[others] = np.array(["B", "C", "D"])[rng.integers(0, 3, others.size)]
    out = np.ma.masked_array(one, mask=~in_a)
    run = lambda lab: regional_totals(models.occu_rn, posterior, **data, regions=lab, weights=w, probs=PROBS, random_seed=6, **opts)
    a, b, c = run(one), run(three), run(out)
    assert list(a["regions"]) == ["A", "B"] and list(b["regions"]) == ["A", "B", "C", "D"] and list(c["regions"]) == ["A"]
    for site in ("abundance", "N_i"):
        rows = [np.ascontiguousarray(r[site]["draws"][..., 0, :]).tobytes() for r in (a, b, c)]
        assert rows[0] == rows[1] == rows[2], site
    # "all" is the sum of a partition's rows, within the bound of the whole
    preds = predict(models.occu_rn, posterior, **data, num_samples=3, random_seed=6, **opts)
    whole = run(None)
    for site, v in (("abundance", f32(preds["abundance"])[:, 0]), ("N_i", np.asarray(preds["N_i"]))):
        _, bound = totals_ref.totals(v, [np.arange(N)], w)
        assert np.all(np.abs(whole[site]["draws"] - b[site]["draws"].sum(axis=-2, keepdims=True)) <= bound), site


# ------------------------------------------------------------------------------------------ weights ----
def test_zero_negative_and_unit_weights():
    data, posterior, opts = _case("nmixture", 60, N=130, max_abundance=5)
    lab = np.random.default_rng(61).integers(0, 2, 130)
    run = lambda w: regional_totals(models.nmixture, posterior, **data, regions=lab, weights=w, probs=PROBS, random_seed=2, **opts)
    zero = run(np.zeros(130))
    assert not zero["abundance"]["draws"].any() and not zero["N_i"]["draws"].any() and list(zero["weight"]) == [0.0, 0.0]
    unit, ones = run(None), run(np.ones(130))
    for site in ("abundance", "N_i"):
        assert unit[site]["draws"].tobytes() == ones[site]["draws"].tobytes(), site
    minus = run(-np.ones(130))
    assert np.array_equal(minus["N_i"]["draws"], -unit["N_i"]["draws"]) and np.all(minus["abundance"]["draws"] < 0)
    _compare("nmixture", data, posterior, opts, regions=lab, weights=np.linspace(-2.0, 1.0, 130), seed=2, label="negative weights")


# ------------------------------------------------------------------------------------------ determinism and outputs ----
def _abi(ds, draws, region, G, weight=None, seed=0, which=(0, 1)):
    """bl_regional_totals through ctypes with only the outputs ``which`` passed; the others stay untouched (-7)."""
    n = draws.shape[0]
    r32 = np.ascontiguousarray(region, dtype=np.int32)
    out = [np.full((n, max(G, 1)), -7.0), np.full((n, ds.T, max(G, 1)), -7.0)]
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    rc = ds._lib.bl_regional_totals(ds._h, n, draws.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint64(seed), G,
                                    r32.ctypes.data_as(C.POINTER(C.c_int32)), dp(weight), *[dp(a) if k in which else None for k, a in enumerate(out)])
    return rc, out


def test_same_bytes_twice_each_output_alone_another_seed_and_the_first_draws():
    data, posterior, opts = _case("occu", 70, N=300, n=40)
    ds, draws = _handle("occu", data, posterior, opts)
    lab = np.random.default_rng(71).integers(-1, 4, 300)
    w = np.random.default_rng(72).uniform(0.1, 2.0, 300)
    rc, a = _abi(ds, draws, lab, 4, w, seed=1)
    assert rc == 0 and all(not (x == -7.0).any() for x in a)
    rc, b = _abi(ds, draws, lab, 4, w, seed=1)
    assert rc == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for k in range(2):
        rc, alone = _abi(ds, draws, lab, 4, w, seed=1, which=[k])
        assert rc == 0 and alone[k].tobytes() == a[k].tobytes() and (alone[1 - k] == -7.0).all(), k
    rc, other = _abi(ds, draws, lab, 4, w, seed=2)
    assert rc == 0 and other[0].tobytes() == a[0].tobytes() and not np.array_equal(other[1], a[1])
    rc, few = _abi(ds, np.ascontiguousarray(draws[:7]), lab, 4, w, seed=1)
    assert rc == 0 and few[0].tobytes() == a[0][:7].tobytes() and few[1].tobytes() == a[1][:7].tobytes()
    # the engine's method: the same arrays, None where not wanted
    m = ds.regional_totals(draws, lab, 4, weight=w, seed=1)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(m, a))
    assert ds.regional_totals(draws, lab, 4, latent=False)[1] is None and ds.regional_totals(draws, lab, 4, site=False)[0] is None
    # a region without a site is 0
    rc, gap = _abi(ds, draws, np.where(lab == 2, -1, lab), 4, w, seed=1)
    assert rc == 0 and not gap[0][:, 2].any() and not gap[1][:, :, 2].any() and gap[0][:, 3].tobytes() == a[0][:, 3].tobytes()
    ds.close()


# ------------------------------------------------------------------------------------------ a real fit ----
def test_a_small_fit():
    with contextlib.redirect_stdout(io.StringIO()):
        data, _ = simulate(n_sites=60, random_seed=1)
    res = fit(models.occu, **data, num_chains=1, num_samples=100, num_warmup=100, timeout=600)
    rng = np.random.default_rng(80)
    N, T, J, Ko = (500,) + np.shape(data["obs_covs"])[1:]
    new = dict(site_covs=f32(rng.normal(size=(N, np.shape(data["site_covs"])[1]))), obs_covs=f32(rng.normal(size=(N, T, J, Ko))))
    lab = np.array(["north", "south", "east", "west"])[rng.integers(0, 4, N)]
    area = rng.uniform(0.5, 2.0, N)
    preds = predict(models.occu, res.mcmc, **new, num_samples=100, random_seed=7)
    got = regional_totals(models.occu, res.mcmc, **new, regions=lab, weights=area, random_seed=7)
    totals_ref.check(got, preds, "psi", "z", lab, area, (0.05, 0.5, 0.95), "fit")
    assert got["n_draws"] == 100 and list(got["regions"]) == ["east", "north", "south", "west"]
    for site in ("psi", "z"):
        assert all(np.isfinite(got[site][k]).all() for k in ("draws", "mean", "sd", "quantiles")), site
        q = got[site]["quantiles"]
        assert np.all(q[0] <= q[1]) and np.all(q[1] <= q[2]) and np.all(q >= 0) and np.all(q <= got["weight"][:, None])
    only = regional_totals(models.occu, res.mcmc, **new, regions=lab, weights=area, latent=False)
    assert "z" not in only and only["psi"]["draws"].tobytes() == got["psi"]["draws"].tobytes()


# ------------------------------------------------------------------------------------------ the C-ABI's refusals ----
def test_refusals_at_the_abi():
    rng = np.random.default_rng(0)
    X, W = f32(rng.normal(size=(20, 1))), f32(rng.normal(size=(20, 2, 2, 1)))
    Y = f32(rng.random((1, 20, 2, 2)) < 0.4)
    blank = lambda J: np.full((1, 20, 2, J), np.nan, dtype=np.float32)
    lab = np.arange(20) % 3
    refused = {"occu_dyn": OccuDataset(X, W, Y, model="occu_dyn"),
               "occu_comb": OccuDataset(X, W, blank(2), model="occu_comb", ARU_obs_covs=rng.normal(size=(20, 2, 3, 1)), ARU_obs=blank(3),
                                        scores_obs=blank(2))}
    for name, ds in refused.items():
        dr = np.zeros((2, ds.D), dtype=np.float32)
        rc, out = _abi(ds, dr, lab, 3)
        assert rc == _ffi.BL_ERR_UNSUPPORTED and b"bl_regional_totals: not built for " + name.encode() in ds._lib.bl_last_error(), name
        assert all((x == -7.0).all() for x in out), name
        with pytest.raises(NotImplementedError):
            ds.regional_totals(dr, lab, 3)
        ds.close()
    ds = OccuDataset(X, W, Y)
    dr = np.zeros((3, ds.D), dtype=np.float32)
    last = ds._lib.bl_last_error
    for bad, G in ((3, 3), (-2, 3)):   # label G, label -2
        rc, out = _abi(ds, dr, np.where(np.arange(20) == 11, bad, lab), G)
        assert rc == _ffi.BL_ERR_INVALID and b"region[11]=%d outside -1 .. n_regions - 1 = 2" % bad in last(), bad
        assert all((x == -7.0).all() for x in out), bad
    w = np.ones(20)
    w[4] = np.nan
    rc, out = _abi(ds, dr, lab, 3, w)
    assert rc == _ffi.BL_ERR_INVALID and b"weight[4]=nan is not finite" in last() and all((x == -7.0).all() for x in out)
    w[4] = np.inf
    rc, out = _abi(ds, dr, lab, 3, w)
    assert rc == _ffi.BL_ERR_INVALID and b"weight[4]=inf" in last() and all((x == -7.0).all() for x in out)
    rc, out = _abi(ds, dr, lab, 3, which=())                # both outputs NULL
    assert rc == _ffi.BL_ERR_INVALID and all((x == -7.0).all() for x in out)
    rc, out = _abi(ds, dr, np.full(20, -1), 0)              # n_regions = 0
    assert rc == _ffi.BL_ERR_INVALID and b"n_regions=0" in last() and all((x == -7.0).all() for x in out)
    with pytest.raises(ValueError):
        ds.regional_totals(dr, lab[:5], 3)
    with pytest.raises(ValueError):
        ds.regional_totals(dr, lab, 3, site=False, latent=False)
    # every site in no region: the totals are zeros
    rc, out = _abi(ds, dr, np.full(20, -1), 2)
    assert rc == 0 and not out[0].any() and not out[1].any()
    # a NUTS launch in flight
    ds.launch(num_warmup=200000, num_samples=200000, num_chains=2, seed=0)
    rc, out = _abi(ds, dr, lab, 3)
    assert rc == _ffi.BL_ERR_BUSY and b"in flight" in last() and all((x == -7.0).all() for x in out)
    ds.abort()
    with pytest.raises(Exception, match="aborted"):
        ds.wait()
    rc, out = _abi(ds, dr, lab, 3)
    assert rc == 0 and not (out[0] == -7.0).any()           # the handle stays usable
    ds.close()
