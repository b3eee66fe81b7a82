"""information_criteria on the GPU: the fused reductions (bl_predictive_density) against a float64 restatement of their definition on
predict()'s arrays for the same seed (z, psi, prob_detection; the rate of the posterior), reduced with scipy's logsumexp and
np.var(ddof=1) -- for both forms and every served handle; two species; the geometry (one site, a tail block, fewer draws than strips,
more draws than grid rows); the masks; the same bytes twice and each output alone; the existing host functions (evaluation.waic /
deviance and their *_manual forms), which is the contract; a small real fit; the refusals at the C-ABI.

Posteriors are hand-made (random float32 coefficients behind a ``get_samples()`` stub); one fit of 60 sites, 100 + 100 draws.

Tolerances.  The oracle's inputs are bit-equal to what the kernels regenerate, so what remains is libm's log / exp (a few float64 ulp) and
the merge order over at most ~1100 draws of |ll| <= 87.4:
  point_lse     |got - want| <= 1e-9 |want| + 1e-9
  point_var     |got - want| <= 1e-9 |want| + 1e-8     (n 2^-52 87.4^2 ~ 2e-9 for n = 1100, with a margin of 5)
  log_lik_draw  rtol 1e-10                             (the order of at most 10^4 additions)
  lppd, p_waic  the sum of their points' bounds;  deviance  2 max |log_lik_draw| 1e-10  (log-sum-exp is 1-Lipschitz)
Against the host functions: rtol 1e-5 on each total for the conditional form without a false-positive rate (the host evaluates log in
float32), rtol 1e-10 for the marginal form (float64 on both sides from the same float32 psi and p).

The false-positive rate.  The C-ABI carries a draw's coordinate phi = float32(logit(rate)), not the rate, and the kernels use the float32
site value of that coordinate, (float)(1 / (1 + exp(-(double)phi))) -- what the layout's sigmoid transform gives a fit's posterior.  A
hand-made float32 rate does not survive the float32 logit bit for bit (it comes back within about 1e-7, a hundred times the bound), so
the oracle takes the posterior's rate through the same coordinate (``_engine_rate``): its inputs are then bit-equal as for psi and p."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest
from scipy.special import logsumexp

from biolith_amd import _ffi
from biolith_amd.engine import OccuDataset
from biolith_amd.evaluation import deviance, deviance_manual, lppd_manual, waic, waic_manual
from biolith_amd.evaluation.predictive_density import _valid_obs
from biolith_amd.models import occu, simulate
from biolith_amd.utils import fit, information_criteria, predict

pytestmark = pytest.mark.gpu

FORMS = ["conditional", "marginal"]
TINY, ONE_MINUS_EPS = float(np.finfo(np.float32).tiny), float(np.float32(1.0) - np.float32(np.finfo(np.float32).eps))


class _Posterior:
    """What predict and information_criteria read of a fit: ``get_samples()``."""

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


def _engine_rate(rate):
    """The posterior's rate as the engine's coordinate carries it: float32 logit, float64 sigmoid, float32 (see the module's docstring)."""
    v = np.clip(np.asarray(rate, dtype=np.float64), 1e-300, 1 - 1e-16)
    phi = np.log(v / (1.0 - v)).astype(np.float32).astype(np.float64)
    return (1.0 / (1.0 + np.exp(-phi))).astype(np.float32).astype(np.float64)


def _oracle(preds, posterior, data, form):
    """The definition in float64 on predict()'s arrays -> lppd_i, p_waic_i (S, N, T, J; NaN off the points), log_lik_draw (n,)."""
    valid = _valid_obs(data["site_covs"], data["obs_covs"], data["obs"])                  # (S, N, T, J)
    y = np.where(valid, np.asarray(data["obs"], dtype=np.float64), 0.0).transpose((3, 2, 1, 0))[None]     # (1, J, T, N, S)
    r = np.asarray(preds["prob_detection"], dtype=np.float32).astype(np.float64)          # (n, J, T, N, S)
    n = r.shape[0]
    if form == "marginal":
        q = np.asarray(preds["psi"], dtype=np.float32).astype(np.float64)[:, None] * r
        ll = y * np.log(np.clip(q, 1e-10, 1 - 1e-10)) + (1.0 - y) * np.log(np.clip(1.0 - q, 1e-10, 1 - 1e-10))
    else:
        z = np.asarray(preds["z"], dtype=np.float64)[:, None]
        prob = z * r
        for mode in ("constant", "unoccupied"):
            if f"prob_fp_{mode}" in posterior.sites:
                f = _engine_rate(posterior.sites[f"prob_fp_{mode}"]).reshape((n,) + (1,) * 4)
                f_c, f_u = (f, 0.0) if mode == "constant" else (0.0, f)
                prob = 1.0 - (1.0 - z * r) * (1.0 - f_c) * (1.0 - (1.0 - z) * f_u)
        prob = np.clip(prob, TINY, ONE_MINUS_EPS)
        ll = y * np.log(prob) + (1.0 - y) * np.log1p(-prob)
    ll = ll.transpose((0, 4, 3, 2, 1))                                                     # (n, S, N, T, J)
    lppd_i = np.where(valid, logsumexp(ll, axis=0) - np.log(n), np.nan)
    var = np.var(ll, axis=0, ddof=1) if n > 1 else np.full(ll.shape[1:], np.nan)
    return lppd_i, np.where(valid, var, np.nan), np.where(valid[None], ll, 0.0).sum(axis=(1, 2, 3, 4)), valid


def _check(got, want, label=""):
    """One fused result against the oracle's, at the bounds of the module's docstring; prints the largest errors."""
    lppd_i, p_waic_i, per_draw, valid = want
    n = per_draw.shape[0]
    assert got["n_points"] == int(valid.sum())
    assert got["lppd_i"].shape == got["p_waic_i"].shape == valid.shape and got["lppd_i"].dtype == got["p_waic_i"].dtype == np.float64
    assert got["log_lik_draw"].shape == (n,) and got["log_lik_draw"].dtype == np.float64
    assert np.isnan(got["lppd_i"][~valid]).all() and np.isnan(got["p_waic_i"][~valid]).all()
    assert np.isfinite(got["lppd_i"][valid]).all()
    e_lse = np.abs(got["lppd_i"][valid] - lppd_i[valid])
    b_lse = 1e-9 * np.abs(lppd_i[valid]) + 1e-9
    if n > 1:
        e_var = np.abs(got["p_waic_i"][valid] - p_waic_i[valid])
        b_var = 1e-9 * np.abs(p_waic_i[valid]) + 1e-8
    else:
        assert np.isnan(got["p_waic_i"]).all() and (np.isnan(got["p_waic"]) or not valid.any())
        e_var, b_var = np.zeros(0), np.zeros(0)
    scale = np.abs(per_draw)
    e_draw = np.abs(got["log_lik_draw"] - per_draw)
    worst = dict(lse=float(np.max(e_lse / b_lse, initial=0.0)), var=float(np.max(e_var / b_var, initial=0.0)),
                 draw=float(np.max(e_draw / np.where(scale > 0, scale, 1.0), initial=0.0)))
    print(f"{label:40s} n {n:5d} points {valid.sum():6d}  max |err| lse {np.max(e_lse, initial=0.0):.2e} ({worst['lse']:.2e} of its bound)  "
          f"var {np.max(e_var, initial=0.0):.2e} ({worst['var']:.2e} of its bound)  log_lik_draw rel {worst['draw']:.2e}")
    assert np.all(e_lse <= b_lse), f"point_lse {label}"
    assert np.all(e_var <= b_var), f"point_var {label}"
    np.testing.assert_allclose(got["log_lik_draw"], per_draw, rtol=1e-10, atol=0, err_msg=f"log_lik_draw {label}")
    # the totals: the sum of the points' bounds; the deviance through the 1-Lipschitz log-sum-exp
    assert got["lppd"] == float(np.sum(got["lppd_i"][valid]))
    assert abs(got["lppd"] - np.sum(lppd_i[valid])) <= np.sum(b_lse) + 1e-300
    if n > 1:
        assert got["p_waic"] == float(np.sum(got["p_waic_i"][valid]))
        assert abs(got["p_waic"] - np.sum(p_waic_i[valid])) <= np.sum(b_var) + 1e-300
        assert got["waic"] == -2 * (got["lppd"] - got["p_waic"])
    want_dev = -2.0 * (logsumexp(per_draw) - np.log(n))
    assert abs(got["deviance"] - want_dev) <= 2e-10 * np.max(scale, initial=0.0) + 1e-12 * abs(want_dev)


def _compare(data, posterior, opts, seed=5, forms=FORMS, label=""):
    """Both forms against the oracle on predict()'s arrays, same seed; returns the fused results by form and predict()'s arrays."""
    n = posterior.sites["beta"].shape[0]
    preds = predict(occu, posterior, **data, num_samples=n, random_seed=seed, **opts)
    out = {}
    for form in forms:
        got = information_criteria(occu, posterior, **data, form=form, pointwise=True, random_seed=seed, **opts)
        _check(got, _oracle(preds, posterior, data, form), f"{label} {form}")
        out[form] = got
    return out, preds


def _against_the_host_functions(out, preds, data):
    """The contract: evaluation.waic / deviance (rtol 1e-5: float32 log on the host) and the *_manual forms (rtol 1e-10)."""
    host = {**waic(occu, preds, **data), "deviance": deviance(occu, preds, **data)}
    manual = {**waic_manual(preds, data), "deviance": deviance_manual(preds, data)}
    assert manual["lppd"] == lppd_manual(preds, data)
    for form, want, rtol in (("conditional", host, 1e-5), ("marginal", manual, 1e-10)):
        for k in ("waic", "lppd", "p_waic", "deviance"):
            print(f"{form:12s}{k:9s} fused {out[form][k]:.12g}  host {want[k]:.12g}  rel {abs(out[form][k] - want[k]) / abs(want[k]):.2e}")
            np.testing.assert_allclose(out[form][k], want[k], rtol=rtol, atol=0, err_msg=f"{form} {k}")


# ------------------------------------------------------------------------------------------ against the oracle and the host ----
def test_block_and_strip_tails():
    # one full 256-site block and a 44-site tail, two periods
    data, posterior, opts = _case(0, N=300, T=2, J=3, n=64)
    out, preds = _compare(data, posterior, opts, label="N=300")
    _against_the_host_functions(out, preds, data)


@pytest.mark.parametrize("N", [1, 257])
def test_one_site_and_one_site_past_a_block(N):
    _compare(*_case(3, N=N, T=2, J=2, n=16), label=f"N={N}")


@pytest.mark.parametrize("n", [1, 2, 3])
def test_fewer_draws_than_strips(n):
    out, _ = _compare(*_case(4, N=40, T=1, J=3, n=n), label=f"n={n}")
    for form in FORMS:
        assert np.isnan(out[form]["p_waic"]) == (n == 1) and np.isfinite(out[form]["lppd"]) and np.isfinite(out[form]["deviance"])


def test_more_draws_than_grid_rows():
    data, posterior, opts = _case(4, N=40, T=1, J=3, n=1100)   # the per-draw loop strides past grid_y = 1024; strips of 18 and 17 draws
    out, preds = _compare(data, posterior, opts, label="n=1100")
    _against_the_host_functions(out, preds, data)


@pytest.mark.parametrize("options", [dict(fp="constant"), dict(fp="unoccupied"), dict(site_re=True, obs_re=True)],
                         ids=["fp_constant", "fp_unoccupied", "random_effects"])
def test_the_other_served_handles(options):
    data, posterior, opts = _case(1, N=70, T=1, J=4, n=32, **options)
    out, preds = _compare(data, posterior, opts, label=str(options))
    if "fp" not in options:   # (with a rate the host forms prob_detection_fp in float32: the oracle alone)
        _against_the_host_functions(out, preds, data)


def test_two_species():
    data, posterior, opts = _case(2, N=40, T=1, J=3, n=32, S=2)
    both, preds = _compare(data, posterior, opts, seed=9, label="S=2")
    _against_the_host_functions(both, preds, data)
    # the plate is summed: species 0 alone is a part of it (its seed is the call's), bit for bit
    one = _Posterior({k: v[:, :1] for k, v in posterior.sites.items()})
    for form in FORMS:
        first = information_criteria(occu, one, **{**data, "obs": data["obs"][:1]}, form=form, pointwise=True, random_seed=9)
        assert first["lppd_i"].tobytes() == both[form]["lppd_i"][:1].tobytes()
        assert first["p_waic_i"].tobytes() == both[form]["p_waic_i"][:1].tobytes()
        assert first["n_points"] < both[form]["n_points"] and np.all(first["log_lik_draw"] > both[form]["log_lik_draw"])


# ------------------------------------------------------------------------------------------ masks ----
def test_masks():
    data, posterior, opts = _case(6, N=70, T=2, J=3, n=32)
    data["obs"][:, :, 1, 2] = np.nan   # one visit never seen
    data["obs"][:, 11] = np.nan        # one site never seen
    data["site_covs"][4, 1] = data["obs_covs"][7, 1, 2, 0] = data["obs_covs"][69, 0, 0, 1] = np.nan
    valid = _valid_obs(data["site_covs"], data["obs_covs"], data["obs"])
    seen = np.isfinite(data["obs"])
    assert not valid[:, 4].any() and not valid[0, 7, 1, 2] and not valid[0, 69, 0, 0] and valid.sum() < seen.sum()
    with_holes, _ = _compare(data, posterior, opts, label="masks")
    # the covariates' NaN read as zero and the same points masked through obs: the same bytes
    filled = dict(site_covs=np.nan_to_num(data["site_covs"]), obs_covs=np.nan_to_num(data["obs_covs"]),
                  obs=np.where(valid, data["obs"], np.nan).astype(np.float32))
    for form, want in with_holes.items():
        assert want["n_points"] == int(valid.sum())
        got = information_criteria(occu, posterior, **filled, form=form, pointwise=True, random_seed=5)
        for k in ("lppd_i", "p_waic_i", "log_lik_draw"):
            assert got[k].tobytes() == want[k].tobytes(), k
        assert (got["lppd"], got["p_waic"], got["waic"], got["deviance"], got["n_points"]) == \
               (want["lppd"], want["p_waic"], want["waic"], want["deviance"], want["n_points"])
    # nothing valid at all
    for form in FORMS:
        none = information_criteria(occu, posterior, **{**data, "obs": np.full(data["obs"].shape, np.nan, np.float32)}, form=form,
                                    pointwise=True)
        assert none["lppd"] == 0.0 and none["n_points"] == 0 and not none["log_lik_draw"].any() and np.isnan(none["lppd_i"]).all()


# ------------------------------------------------------------------------------------------ determinism and outputs ----
def _handle(data):
    return OccuDataset(data["site_covs"], data["obs_covs"], np.full(data["obs"][:1].shape, np.nan, dtype=np.float32))


def test_same_bytes_twice_and_each_output_alone():
    data, posterior, _ = _case(5, N=300, T=2, J=3, n=40)
    ds = _handle(data)
    th = np.concatenate([posterior.sites["beta"][:, 0], posterior.sites["alpha"][:, 0]], axis=1)
    obs = data["obs"][0]
    for marginal in (False, True):
        a, b, c = (ds.predictive_density(th, obs, seed=s, marginal=marginal) for s in (7, 7, 8))
        assert [x.shape for x in a] == [(40,), (300, 2, 3), (300, 2, 3)] and all(x.dtype == np.float64 for x in a)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        # another seed: another z in the conditional form; the marginal form draws nothing
        assert all((x.tobytes() == y.tobytes()) == marginal for x, y in zip(a, c))
        assert not a[1][np.isnan(obs)].any() and not a[2][np.isnan(obs)].any() and a[1][np.isfinite(obs)].all()
        for k in range(3):
            alone = ds.predictive_density(th, obs, seed=7, marginal=marginal, per_draw=k == 0, point_lse=k == 1, point_var=k == 2)
            assert [x is None for x in alone] == [j != k for j in range(3)] and alone[k].tobytes() == a[k].tobytes()
        # a function of (seed, draw, period, site): the first draws of a longer call are the shorter call
        head = ds.predictive_density(th[:7], obs, seed=7, marginal=marginal)
        assert head[0].tobytes() == a[0][:7].tobytes()
    with pytest.raises(ValueError, match="0, 1 or NaN"):
        ds.predictive_density(th, np.where(np.isnan(obs), np.nan, 2.0), seed=7)
    with pytest.raises(ValueError, match="shape"):
        ds.predictive_density(th, obs[:, :, :2], seed=7)
    with pytest.raises(ValueError):
        ds.predictive_density(th, obs, per_draw=False, point_lse=False, point_var=False)
    ds.close()


def test_the_seed_moves_the_conditional_form_only():
    data, posterior, opts = _case(8, N=70, T=2, J=3, n=32)
    for form in FORMS:
        a, b = (information_criteria(occu, posterior, **data, form=form, pointwise=True, random_seed=s) for s in (1, 2))
        same = all(a[k].tobytes() == b[k].tobytes() for k in ("lppd_i", "p_waic_i", "log_lik_draw")) and a["waic"] == b["waic"]
        assert same == (form == "marginal")


# ------------------------------------------------------------------------------------------ a real fit ----
def test_a_small_fit():
    with contextlib.redirect_stdout(io.StringIO()):
        data, _ = simulate(n_sites=60, random_seed=1)
    res = fit(occu, **data, num_chains=1, num_samples=100, num_warmup=100, timeout=600)
    preds = predict(occu, res.mcmc, **data, num_samples=100, random_seed=3)
    out = {form: information_criteria(occu, res.mcmc, **data, form=form, random_seed=3) for form in FORMS}
    for got in out.values():
        assert all(np.isfinite(got[k]) for k in ("waic", "lppd", "p_waic", "deviance")) and np.isfinite(got["log_lik_draw"]).all()
        assert got["waic"] == -2 * (got["lppd"] - got["p_waic"]) and "lppd_i" not in got
        assert got["n_points"] == int(_valid_obs(data["site_covs"], data["obs_covs"], data["obs"]).sum())
    _against_the_host_functions(out, preds, {k: data[k] for k in ("site_covs", "obs_covs", "obs")})


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
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    for name, ds in handles.items():
        lib = ds._lib
        dr = np.zeros((n, ds.D), dtype=np.float32)
        fp = dr.ctypes.data_as(C.POINTER(C.c_float))
        obs = np.zeros(ds.J * ds.T * ds.N, dtype=np.uint8)
        po = obs.ctypes.data_as(C.POINTER(C.c_uint8))
        per_draw, points = np.zeros(n), np.zeros((2, obs.size))
        assert lib.bl_predictive_density(ds._h, n, fp, 0, po, 0, dp(per_draw), dp(points[0]), dp(points[1])) == _ffi.BL_ERR_UNSUPPORTED
        assert b"bl_predictive_density: not built for " + name.encode() in lib.bl_last_error()
        assert lib.bl_predictive_density(ds._h, n, fp, 0, po, 0, None, None, None) == _ffi.BL_ERR_INVALID
        assert not per_draw.any() and not points.any()
        with pytest.raises(NotImplementedError, match=name):
            ds.predictive_density(dr, np.zeros((ds.N, ds.T, ds.J)))
        ds.close()
    # a served handle: all outputs NULL, no observations, or a byte that is no observation, is a bad argument
    ds = OccuDataset(data["site_covs"], data["obs_covs"], data["obs"])
    dr = np.zeros((n, ds.D), dtype=np.float32)
    fp = dr.ctypes.data_as(C.POINTER(C.c_float))
    obs = np.zeros(ds.J * ds.T * ds.N, dtype=np.uint8)
    po = obs.ctypes.data_as(C.POINTER(C.c_uint8))
    per_draw, points = np.zeros(n), np.zeros((2, obs.size))
    call = ds._lib.bl_predictive_density
    assert call(ds._h, n, fp, 0, po, 0, None, None, None) == _ffi.BL_ERR_INVALID
    assert call(ds._h, n, fp, 0, None, 0, dp(per_draw), None, None) == _ffi.BL_ERR_INVALID
    obs[3] = 7
    for marginal in (0, 1):
        assert call(ds._h, n, fp, 0, po, marginal, dp(per_draw), dp(points[0]), dp(points[1])) == _ffi.BL_ERR_INVALID
        assert b"obs holds 7" in ds._lib.bl_last_error()
    assert not per_draw.any() and not points.any()
    ds.close()
