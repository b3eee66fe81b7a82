"""predictive_check on the GPU: the fused check (bl_predictive_check) against the host path -- posterior_predictive_check's own float64
expressions on predict()'s arrays for the same seed -- for every grouping and statistic and every served handle; two species; the
geometry (one site, a tail block, more draws than grid rows, the same bytes twice, one output without the other); missing revisits,
sites and covariates; a small real fit; the refusals at the C-ABI.

Posteriors are hand-made (random float32 coefficients behind a ``get_samples()`` stub); one fit of 60 sites, 100 + 100 draws.

Tolerance: the replicate is predict()'s bit for bit and E = psi * p is exact in float64, so only the order of at most ~10^4 non-negative
float64 additions differs: rtol 1e-10 (count x 2^-53 ~ 1e-12).  The p-value is compared exactly."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest

from biolith_amd import _ffi
from biolith_amd.engine import OccuDataset
from biolith_amd.evaluation import posterior_predictive_check
from biolith_amd.models import occu, simulate
from biolith_amd.utils import fit, predict, predictive_check

pytestmark = pytest.mark.gpu

RTOL = 1e-10
PAIRS = [(g, s) for g in ("site", "revisit") for s in ("freeman-tukey", "chi-squared")]


class _Posterior:
    """What predict and predictive_check read of a fit: ``get_samples()``."""

    def __init__(self, sites):
        self.sites = sites

    def get_samples(self):
        return self.sites


def _case(seed, N, T, J, n, Ks=2, Ko=2, S=1, missing=0.1, fp=None, site_re=False, obs_re=False):
    """Random data with ``missing`` of obs NaN, a hand-made posterior for it, and the model options."""
    rng = np.random.default_rng(seed)
    data = dict(site_covs=rng.normal(size=(N, Ks)).astype(np.float32), obs_covs=rng.normal(size=(N, T, J, Ko)).astype(np.float32))
    obs = (rng.random((S, N, T, J)) < 0.35).astype(np.float32)
    obs[rng.random(obs.shape) < missing] = np.nan
    data["obs"] = obs
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    sites = dict(beta=f32(rng.uniform(-1, 1, (n, S, Ks + 1))), alpha=f32(rng.uniform(-1, 1, (n, S, Ko + 1))))
    opts = {}
    if fp:
        opts[f"false_positives_{fp}"] = True
        sites[f"prob_fp_{fp}"] = f32(rng.uniform(0.05, 0.3, n))
    if site_re:
        opts["site_random_effects"] = True
        sites.update(site_re_sd=f32(rng.uniform(0.3, 1.0, n)), site_re_occ=f32(rng.normal(0, 0.5, (n, N, S))),
                     site_re_det=f32(rng.normal(0, 0.5, (n, N, S))))
    if obs_re:
        opts["obs_random_effects"] = True
        sites.update(obs_re_sd=f32(rng.uniform(0.3, 1.0, n)), obs_re=f32(rng.normal(0, 0.5, (n, J, T, N, S))))
    return data, _Posterior(sites), opts


def _host(preds, obs, group_by, statistic):
    """d_obs, d_rep (n,) by the float64 expressions of evaluation.posterior_predictive_check, in its order."""
    stat = {"freeman-tukey": lambda o, e: (np.sqrt(o) - np.sqrt(e)) ** 2, "chi-squared": lambda o, e: (o - e) ** 2 / (e + 1e-10)}[statistic]
    obs = np.asarray(obs, dtype=np.float64)
    y_rep = np.asarray(preds["y"], dtype=np.float64).transpose((0, 4, 3, 2, 1))
    p = np.asarray(preds["prob_detection"], dtype=np.float64).transpose((0, 4, 3, 2, 1))
    psi = np.asarray(preds["psi"], dtype=np.float64)
    expected = psi.transpose((0, 3, 2, 1))[..., None] * p
    seen = np.isfinite(obs)[None]
    axes_obs, axes_rep = ((2, 3), (3, 4)) if group_by == "site" else ((1,), (2,))
    obs_g = np.nansum(obs, axis=axes_obs)
    rep_g = np.where(seen, y_rep, 0.0).sum(axis=axes_rep)
    exp_g = np.where(seen, expected, 0.0).sum(axis=axes_rep)
    axes = tuple(range(1, exp_g.ndim))
    return stat(obs_g[None], exp_g).sum(axis=axes), stat(rep_g, exp_g).sum(axis=axes)


def _compare(data, posterior, opts, seed=5, pairs=PAIRS):
    """The fused check against the host path on predict()'s arrays, same seed; returns the fused results by pair."""
    n = posterior.sites["beta"].shape[0]
    preds = predict(occu, posterior, **data, num_samples=n, random_seed=seed, **opts)
    out = {}
    for g, s in pairs:
        got = predictive_check(occu, posterior, **data, group_by=g, statistic=s, random_seed=seed, **opts)
        d_obs, d_rep = _host(preds, data["obs"], g, s)
        assert got["d_obs"].shape == got["d_rep"].shape == (n,) and got["d_obs"].dtype == got["d_rep"].dtype == np.float64
        err = max(np.max(np.abs(got[k] - w) / np.abs(w)) for k, w in (("d_obs", d_obs), ("d_rep", d_rep)))
        print(f"{g:8s}{s:14s} max rel err {err:.3e}  p {got['p_value']:.4f}")
        np.testing.assert_allclose(got["d_obs"], d_obs, rtol=RTOL, atol=0, err_msg=f"d_obs {g} {s}")
        np.testing.assert_allclose(got["d_rep"], d_rep, rtol=RTOL, atol=0, err_msg=f"d_rep {g} {s}")
        assert got["p_value"] == posterior_predictive_check(preds, data["obs"], g, s) == float(np.mean(got["d_rep"] > got["d_obs"]))
        out[g, s] = got
    return out


# ------------------------------------------------------------------------------------------ equality with the host path ----
def test_equals_the_host_path():
    # one full 256-site block and a 44-site tail, two periods
    _compare(*_case(0, N=300, T=2, J=3, n=64))


@pytest.mark.parametrize("options", [dict(fp="constant"), dict(fp="unoccupied"), dict(site_re=True, obs_re=True)],
                         ids=["fp_constant", "fp_unoccupied", "random_effects"])
def test_the_other_served_handles(options):
    _compare(*_case(1, N=70, T=1, J=4, n=32, **options))


def test_two_species():
    data, posterior, opts = _case(2, N=40, T=1, J=3, n=32, S=2)
    both = _compare(data, posterior, opts, seed=9)
    # the plate is summed: species 0 alone is a part of it (its seed is the call's)
    one = _Posterior({k: v[:, :1] for k, v in posterior.sites.items()})
    first = predictive_check(occu, one, **{**data, "obs": data["obs"][:1]}, random_seed=9)
    assert np.all(first["d_obs"] < both["site", "freeman-tukey"]["d_obs"]) and np.all(first["d_obs"] > 0)


# ------------------------------------------------------------------------------------------ geometry ----
@pytest.mark.parametrize("N", [1, 257])
def test_one_site_and_one_site_past_a_block(N):
    _compare(*_case(3, N=N, T=2, J=2, n=16))


def _handle(data):
    return OccuDataset(data["site_covs"], data["obs_covs"], np.full(data["obs"][:1].shape, np.nan, dtype=np.float32))


def test_more_draws_than_grid_rows():
    data, posterior, opts = _case(4, N=40, T=1, J=3, n=1100)   # the draw loop strides past grid_y = 1024
    _compare(data, posterior, opts, pairs=[("site", "chi-squared"), ("revisit", "freeman-tukey")])


def test_same_bytes_twice_and_one_output_alone():
    data, posterior, _ = _case(5, N=300, T=2, J=3, n=40)
    ds = _handle(data)
    th = np.concatenate([posterior.sites["beta"][:, 0], posterior.sites["alpha"][:, 0]], axis=1)
    obs = data["obs"][0]
    a, b, c = ds.predictive_check(th, obs, seed=7), ds.predictive_check(th, obs, seed=7), ds.predictive_check(th, obs, seed=8)
    assert [x.shape for x in a] == [(40, 4), (40, 4)] and [x.dtype for x in a] == [np.float64, np.float64]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    # another seed: another replicate, the same observed side
    assert np.array_equal(a[0][:, [0, 2]], c[0][:, [0, 2]]) and not np.array_equal(a[0][:, [1, 3]], c[0][:, [1, 3]])
    site_only, revisit_only = ds.predictive_check(th, obs, seed=7, by_revisit=False), ds.predictive_check(th, obs, seed=7, by_site=False)
    assert site_only[1] is None and revisit_only[0] is None
    assert site_only[0].tobytes() == a[0].tobytes() and revisit_only[1].tobytes() == a[1].tobytes()
    # a function of (seed, draw, period, site): the first draws of a longer call are the shorter call
    head = ds.predictive_check(th[:7], obs, seed=7)
    assert head[0].tobytes() == a[0][:7].tobytes() and head[1].tobytes() == a[1][:7].tobytes()
    with pytest.raises(ValueError, match="0, 1 or NaN"):
        ds.predictive_check(th, np.where(np.isnan(obs), np.nan, 2.0), seed=7)
    with pytest.raises(ValueError, match="shape"):
        ds.predictive_check(th, obs[:, :, :2], seed=7)
    ds.close()


# ------------------------------------------------------------------------------------------ edges ----
def test_a_revisit_and_a_site_never_seen():
    data, posterior, opts = _case(6, N=70, T=2, J=3, n=32)
    data["obs"][:, :, 1, 2] = np.nan   # one revisit never seen
    data["obs"][:, 11] = np.nan        # one site never seen
    _compare(data, posterior, opts)
    # nothing seen at all: both sides are exactly 0, whatever the grouping
    ds = _handle(data)
    th = np.concatenate([posterior.sites["beta"][:, 0], posterior.sites["alpha"][:, 0]], axis=1)
    by_site, by_revisit = ds.predictive_check(th, np.full((70, 2, 3), np.nan), seed=1)
    assert not by_site.any() and not by_revisit.any()
    ds.close()


def test_missing_covariates_read_as_zero():
    data, posterior, opts = _case(7, N=70, T=2, J=3, n=32)
    data["site_covs"][4, 1] = data["obs_covs"][7, 1, 2, 0] = data["obs_covs"][69, 0, 0, 1] = np.nan
    with_holes = _compare(data, posterior, opts)
    filled = {**data, "site_covs": np.nan_to_num(data["site_covs"]), "obs_covs": np.nan_to_num(data["obs_covs"])}
    for (g, s), want in with_holes.items():
        got = predictive_check(occu, posterior, **filled, group_by=g, statistic=s, random_seed=5)
        assert got["d_obs"].tobytes() == want["d_obs"].tobytes() and got["d_rep"].tobytes() == want["d_rep"].tobytes()


# ------------------------------------------------------------------------------------------ a real fit ----
def test_a_small_fit():
    with contextlib.redirect_stdout(io.StringIO()):
        data, _ = simulate(n_sites=60, random_seed=1)
    res = fit(occu, **data, num_chains=1, num_samples=100, num_warmup=100, timeout=600)
    preds = predict(occu, res.mcmc, **data, num_samples=100, random_seed=3)
    for g, s in PAIRS:
        got = predictive_check(occu, res.mcmc, **data, group_by=g, statistic=s, random_seed=3)
        assert 0.0 <= got["p_value"] <= 1.0
        assert got["p_value"] == posterior_predictive_check(preds, data["obs"], g, s)


# ------------------------------------------------------------------------------------------ the C-ABI's refusals ----
def test_refusals_at_the_abi():
    with contextlib.redirect_stdout(io.StringIO()):
        data, _ = simulate(n_sites=20, random_seed=0)
    rng = np.random.default_rng(0)
    blank = lambda J: np.full((1, 20, 2, J), np.nan, dtype=np.float32)
    handles = {"occu_rn": OccuDataset(data["site_covs"], data["obs_covs"], data["obs"], model="occu_rn", max_abundance=20),
               "occu_comb": OccuDataset(rng.normal(size=(20, 1)), rng.normal(size=(20, 2, 2, 1)), blank(2), model="occu_comb",
                                        ARU_obs_covs=rng.normal(size=(20, 2, 3, 1)), ARU_obs=blank(3), scores_obs=blank(2))}
    n = 2
    for name, ds in handles.items():
        lib = ds._lib
        dr = np.zeros((n, ds.D), dtype=np.float32)
        fp = dr.ctypes.data_as(C.POINTER(C.c_float))
        obs = np.zeros(ds.J * ds.T * ds.N, dtype=np.uint8)
        po = obs.ctypes.data_as(C.POINTER(C.c_uint8))
        out = np.zeros((2, n, 4))
        p0, p1 = (o.ctypes.data_as(C.POINTER(C.c_double)) for o in out)
        assert lib.bl_predictive_check(ds._h, n, fp, 0, po, p0, p1) == _ffi.BL_ERR_UNSUPPORTED
        assert b"bl_predictive_check: not built for " + name.encode() in lib.bl_last_error()
        assert lib.bl_predictive_check(ds._h, n, fp, 0, po, None, None) == _ffi.BL_ERR_INVALID
        assert not out.any()
        with pytest.raises(NotImplementedError, match=name):
            ds.predictive_check(dr, np.zeros((ds.N, ds.T, ds.J)))
        ds.close()
    # a served handle: both outputs NULL, or no observations, is a bad argument
    ds = OccuDataset(data["site_covs"], data["obs_covs"], data["obs"])
    dr = np.zeros((n, ds.D), dtype=np.float32)
    fp = dr.ctypes.data_as(C.POINTER(C.c_float))
    obs = np.zeros(ds.J * ds.T * ds.N, dtype=np.uint8)
    po = obs.ctypes.data_as(C.POINTER(C.c_uint8))
    out = np.zeros((n, 4))
    p0 = out.ctypes.data_as(C.POINTER(C.c_double))
    assert ds._lib.bl_predictive_check(ds._h, n, fp, 0, po, None, None) == _ffi.BL_ERR_INVALID
    assert ds._lib.bl_predictive_check(ds._h, n, fp, 0, None, p0, None) == _ffi.BL_ERR_INVALID
    obs[3] = 7
    assert ds._lib.bl_predictive_check(ds._h, n, fp, 0, po, p0, None) == _ffi.BL_ERR_INVALID and b"obs holds 7" in ds._lib.bl_last_error()
    assert not out.any()
    ds.close()
