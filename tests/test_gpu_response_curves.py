"""response_curves on the GPU.  The fused curves (bl_response_curves) against the route that existed before them -- one handle per grid
value on the modified covariates and ``regional_totals`` for one region --, byte for byte on the site side; both sides of every served
handle kind against ``deterministic`` on the modified covariates reduced in the stated order (tests/curves_ref.py), byte for byte; the
independence of a value's column from the other values, across the kernels' block of values; the geometry (one site, sizes around a
wave and a block, a draw loop that strides past the grid rows, a chunk boundary); weights; the normalisers; two species; the same bytes
twice; the wrapper against its docstring contract on ``predict()``'s arrays; the float64 logistic formula; the refusals at the C-ABI.

Posteriors are hand-made (random float32 coefficients in (-1, 1) behind a ``get_samples()`` stub); one fit of 60 sites, 100 + 100
draws.  No tolerance appears at the engine level.  Against ``predict()`` both sides sum the same float64 terms, so the bound is derived
(tests/totals_ref.py): ``2 (N - 1) 2^-53 sum_i |w_i v_i|``, over the normaliser."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest

import curves_ref
from biolith_amd import _ffi, models
from biolith_amd.engine import OccuDataset
from biolith_amd.models import simulate
from biolith_amd.utils import fit, predict, response_curves
from biolith_amd.utils.response_curves import curve_name
from test_gpu_regional_totals import HANDLES, IDS, _case, _handle, _Posterior

pytestmark = pytest.mark.gpu

PROBS = (0.05, 0.5, 0.95)
VALUE_BLOCK = 8   # BL_RC_VALUE_BLOCK of biolith_amd/csrc/response_curves.hpp
f32 = lambda a: np.asarray(a, dtype=np.float32)


def _modified(data, side, k, value):
    """The data with covariate ``k`` of the side set to ``value`` at every site (and visit)."""
    key = "obs_covs" if side else "site_covs"
    a = data[key].copy()
    a[..., k] = value
    return dict(data, **{key: a})


def _terms(name, data, posterior, opts, side, k, value, w):
    """The per-site float64 terms (n, N) of one grid value, from ``deterministic`` of the handle on the modified arrays."""
    ds, draws = _handle(name, _modified(data, side, k, value), posterior, opts)
    psi, pd = ds.deterministic(draws, psi=not side, prob_detection=bool(side))
    ds.close()
    return curves_ref.obs_terms(pd, w) if side else curves_ref.site_terms(psi[:, 0], w)


def _want(name, data, posterior, opts, side, k, values, w=None):
    """(n, V) float64: the curves as the stated order predicts them, byte for byte."""
    return np.stack([curves_ref.ordered_sum(_terms(name, data, posterior, opts, side, k, v, w)) for v in f32(values)], axis=1)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------ the route that exists today ----
@pytest.mark.parametrize("Ks,k", [(3, 0), (3, 1), (3, 2), (1, 0), (16, 15)])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_site_side_equals_regional_totals_on_the_modified_handles(N, Ks, k):
    """n in {1, 3} and V in {1, 5} from the same five handles: column g is ``regional_totals`` of one region on the data whose column
    k holds values[g]."""
    data, posterior, opts = _case("occu", 100 * N + Ks, N=N, n=3, Ks=Ks, J=1, T=1)
    rng = np.random.default_rng(N)
    values, w = f32(rng.normal(size=5) * 2.0), rng.uniform(0.1, 5.0, N)
    ds, draws = _handle("occu", data, posterior, opts)
    old = []
    for v in values:
        other, same_draws = _handle("occu", _modified(data, 0, k, v), posterior, opts)
        assert _same(same_draws, draws)
        old.append(other.regional_totals(draws, np.zeros(N, dtype=np.int32), 1, weight=w, site=True, latent=False)[0][:, 0])
        other.close()
    old = np.stack(old, axis=1)                                                   # (3, 5)
    for n in (1, 3):
        for V in (1, 5):
            got = ds.response_curves(draws[:n], 0, k, values[:V], weight=w)
            assert got.shape == (n, V) and got.dtype == np.float64
            assert _same(got, np.ascontiguousarray(old[:n, :V])), (N, Ks, k, n, V)
    ds.close()


# ------------------------------------------------------------------------------------------ every served model and handle kind ----
@pytest.mark.parametrize("name,options", HANDLES, ids=IDS)
def test_both_sides_of_every_served_handle(name, options):
    rng = np.random.default_rng(21)
    weights = rng.uniform(-1.0, 4.0, 70)
    values = f32([-1.25, 0.0, 0.7])
    for Ko, w in ((1, None), (3, weights)):           # unit weights once
        data, posterior, opts = _case(name, 20 + Ko, N=70, T=2, J=3, n=3, Ks=2, Ko=Ko, **options)
        ds, draws = _handle(name, data, posterior, opts)
        for side, k in [(0, Ko % 2)] + [(1, k) for k in sorted({0, Ko - 1})]:
            got = ds.response_curves(draws, side, k, values, weight=w)
            assert _same(got, _want(name, data, posterior, opts, side, k, values, w)), (name, options, Ko, side, k)
            assert np.isfinite(got).all()
        ds.close()


# ------------------------------------------------------------------------------------------ a value's column is its own ----
@pytest.mark.parametrize("side", [0, 1], ids=["site", "obs"])
def test_a_column_does_not_depend_on_the_other_values(side):
    data, posterior, opts = _case("occu", 31, N=130, T=2, J=2, n=4, Ks=3, Ko=3, site_re=True, obs_re=True)
    ds, draws = _handle("occu", data, posterior, opts)
    w = np.random.default_rng(32).uniform(0.2, 3.0, 130)
    a, b, c = f32([-0.5, 0.3, 1.75])
    three = ds.response_curves(draws, side, 1, [a, b, c], weight=w)
    assert _same(np.ascontiguousarray(three[:, 1:2]), ds.response_curves(draws, side, 1, [b], weight=w))
    assert _same(three, ds.response_curves(draws, side, 1, [a, b, c], weight=w))          # the same bytes on a second call
    # across the block of values a lane holds (the site kernel reduces it together, the obs kernel loads a visit once for it): one short
    # of a block, a block, one past it, two blocks, one past two -- and the grid reversed
    grid = f32(np.random.default_rng(33).normal(size=2 * VALUE_BLOCK + 1))
    alone = np.concatenate([ds.response_curves(draws, side, 1, [v], weight=w) for v in grid], axis=1)
    for V in (VALUE_BLOCK - 1, VALUE_BLOCK, VALUE_BLOCK + 1, 2 * VALUE_BLOCK, 2 * VALUE_BLOCK + 1):
        assert _same(ds.response_curves(draws, side, 1, grid[:V], weight=w), np.ascontiguousarray(alone[:, :V])), (side, V)
    assert _same(ds.response_curves(draws, side, 1, grid[::-1].copy(), weight=w), np.ascontiguousarray(alone[:, ::-1]))
    ds.close()


def test_the_identity():
    """Every site already holds c in column k: values=[c] is ``regional_totals`` on the unmodified data."""
    data, posterior, opts = _case("occu_rn", 41, N=150, n=3, Ks=3)
    c = np.float32(0.625)
    data["site_covs"][:, 2] = c
    ds, draws = _handle("occu_rn", data, posterior, opts)
    w = np.random.default_rng(42).uniform(0.1, 2.0, 150)
    want = ds.regional_totals(draws, np.zeros(150, dtype=np.int32), 1, weight=w, site=True, latent=False)[0]
    assert _same(ds.response_curves(draws, 0, 2, [c], weight=w), want)
    ds.close()


# ------------------------------------------------------------------------------------------ geometry ----
@pytest.mark.parametrize("side", [0, 1], ids=["site", "obs"])
def test_the_draw_loop_strides_past_the_grid_rows(side):
    data, posterior, opts = _case("occu", 12, N=40, n=1100, Ks=2, Ko=2)
    ds, draws = _handle("occu", data, posterior, opts)
    w = np.linspace(-1.0, 2.0, 40)
    values = f32([-0.4, 1.1])
    got = ds.response_curves(draws, side, 1, values, weight=w)
    ds.close()
    assert got.shape == (1100, 2) and _same(got, _want("occu", data, posterior, opts, side, 1, values, w))


def test_a_chunk_boundary():
    """N = 65 536 sites are 1024 runs of 64; with V = 64 values a draw's workspace is 64 x 1024 x 8 bytes = 512 KiB, so 512 draws fill
    the 256 MiB of BL_TOTALS_WORKSPACE_BYTES and 515 draws go through in two chunks, 0 .. 511 and 512 .. 514.  The call equals the two
    calls on the draws before and after the boundary, and the rows on either side of it the stated order, for two values."""
    N, V, n = 65536, 64, 515
    chunk = (256 << 20) // (V * (N // 64) * 8)
    assert chunk == 512 and chunk < n
    data, posterior, opts = _case("occu", 13, N=N, n=n, T=1, J=1)
    ds, draws = _handle("occu", data, posterior, opts)
    rng = np.random.default_rng(3)
    w, values = rng.normal(size=N), f32(rng.normal(size=V))
    got = ds.response_curves(draws, 0, 1, values, weight=w)
    before = ds.response_curves(np.ascontiguousarray(draws[:chunk]), 0, 1, values, weight=w)
    after = ds.response_curves(np.ascontiguousarray(draws[chunk:]), 0, 1, values, weight=w)
    ds.close()
    assert got.shape == (n, V) and _same(got, np.concatenate([before, after]))
    rows = [chunk - 1, chunk]
    edge = _Posterior({key: a[rows] for key, a in posterior.sites.items()})
    for g in (0, V - 1):
        assert _same(np.ascontiguousarray(got[rows, g]), _want("occu", data, edge, opts, 0, 1, values[g:g + 1], w)[:, 0]), g


# ------------------------------------------------------------------------------------------ weights ----
@pytest.mark.parametrize("side", [0, 1], ids=["site", "obs"])
def test_none_zero_and_negative_weights(side):
    N = 130
    data, posterior, opts = _case("nmixture", 60, N=N, n=3, max_abundance=5)
    ds, draws = _handle("nmixture", data, posterior, opts)
    values = f32([-1.0, 0.5])
    run = lambda w: ds.response_curves(draws, side, 0, values, weight=w)
    unit = run(None)
    assert _same(unit, run(np.ones(N))) and _same(unit, _want("nmixture", data, posterior, opts, side, 0, values))
    assert not run(np.zeros(N)).any()
    minus = run(-np.ones(N))
    assert _same(minus, -unit) and np.all(minus < 0)
    w = np.linspace(-2.0, 1.0, N)
    assert _same(run(w), _want("nmixture", data, posterior, opts, side, 0, values, w))
    # zeros at some sites: those sites drop out -- the curve of the remaining sites alone, two float64 sums of the same non-zero terms
    keep = np.random.default_rng(61).random(N) < 0.6
    w0 = np.where(keep, np.random.default_rng(62).uniform(0.5, 2.0, N), 0.0)
    got = run(w0)
    assert _same(got, _want("nmixture", data, posterior, opts, side, 0, values, w0))
    part = {key: a[keep] for key, a in data.items()}
    kept = _Posterior(posterior.sites)
    sub, sub_draws = _handle("nmixture", part, kept, opts)
    assert _same(sub_draws, draws)
    alone = sub.response_curves(draws, side, 0, values, weight=w0[keep])
    sub.close()
    ds.close()
    terms = np.stack([_terms("nmixture", part, kept, opts, side, 0, v, w0[keep]) for v in values], axis=1)   # (n, V, N')
    assert np.all(np.abs(got - alone) <= curves_ref.bound(terms))


# ------------------------------------------------------------------------------------------ the wrapper ----
def _contract(name, data, posterior, opts, side, k, values, weights, label):
    """The wrapper against its docstring: the totals (``average=False``) against ``predict()`` on the modified arrays within the derived
    bound ``2 (N - 1) 2^-53 sum |w v|``, and the averages as those totals over the normaliser, exactly -- the bound scaled by the
    normaliser.  On the obs side ``v`` is the site's float64 sum over the visits in ascending v = t J + j, as the contract states it.
    Returns the averaged result."""
    model = getattr(models, name)
    n = posterior.sites["beta"].shape[0] if isinstance(posterior, _Posterior) else None
    run = lambda average: response_curves(model, posterior, **data, covariate=k, side=side, values=values, weights=weights, average=average,
                                          probs=PROBS, **opts)
    got, tot = run(True), run(False)
    n = got["n_draws"] if n is None else n
    site = curve_name(name, side)
    N, T, J = data["obs_covs"].shape[:3]
    w = np.ones(N) if weights is None else np.asarray(weights, dtype=np.float64)
    scale = w.sum() * (T * J if side == "obs" else 1)
    for r in (got, tot):
        assert set(r) == {"side", "covariate", "values", "n_sites", "weight", "probs", "n_draws", site}, label
        assert r["side"] == side and r["covariate"] == k and r["n_sites"] == N and r["n_draws"] == n and r["weight"] == w.sum()
        assert r["values"].dtype == np.float32 and np.array_equal(r["probs"], PROBS)
    d = tot[site]["draws"]
    V = got["values"].size
    worst = 0.0
    for g, v in enumerate(got["values"]):
        preds = predict(model, posterior, **_modified(data, side == "obs", k, v), num_samples=n, **opts)
        p = f32(preds[site])                                                           # (n, T, N, S) / (n, J, T, N, S)
        for sp in range(p.shape[-1]):
            terms = curves_ref.site_terms(p[:, 0, :, sp], w) if side == "site" else curves_ref.obs_terms(p[..., sp], w)   # (n, N)
            err, bound = np.abs(d[:, g, sp] - terms.sum(axis=1)), curves_ref.bound(terms)
            assert np.all(err <= bound), (label, g, sp, float(err.max()), float(bound.max()))
            worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0)))
    print(f"{label}: largest error {worst:.3g} of its bound")
    assert _same(got[site]["draws"], d / scale), label
    for r in (got, tot):
        e = r[site]["draws"]
        assert e.shape == (n, V, p.shape[-1]) and r[site]["mean"].shape == e.shape[1:] and r[site]["quantiles"].shape == (3,) + e.shape[1:]
        assert np.array_equal(r[site]["mean"], e.mean(axis=0)) and np.array_equal(r[site]["quantiles"], np.quantile(e, PROBS, axis=0))
        assert np.array_equal(r[site]["sd"], e.std(axis=0, ddof=1))
    return got


@pytest.mark.parametrize("name,side", [("occu", "site"), ("occu", "obs"), ("occu_rn", "site"), ("occu_cop", "obs")])
def test_the_wrapper_against_its_contract(name, side):
    data, posterior, opts = _case(name, 70, N=90, T=2, J=2, n=4, Ks=2, Ko=2)
    w = np.random.default_rng(71).uniform(0.5, 2.0, 90)
    got = _contract(name, data, posterior, opts, side, 1, [-1.0, 0.1, 0.9], w, f"{name} {side}")
    assert got["values"].tobytes() == f32([-1.0, 0.1, 0.9]).tobytes()
    _contract(name, data, posterior, opts, side, 0, [0.25], None, f"{name} {side}, unit weights")


@pytest.mark.parametrize("side", ["site", "obs"])
def test_the_normalisers(side):
    data, posterior, opts = _case("occu", 72, N=50, T=2, J=3, n=3)
    w = np.random.default_rng(73).uniform(-0.5, 2.0, 50)
    run = lambda **kw: response_curves(models.occu, posterior, **data, side=side, values=[-0.5, 0.5], probs=PROBS, **kw, **opts)
    site = curve_name("occu", side)
    for weights, total in ((None, 50.0), (w, float(w.sum()))):
        mean, tot = run(weights=weights), run(weights=weights, average=False)
        scale = total * (6 if side == "obs" else 1)
        assert mean["weight"] == tot["weight"] == total
        assert _same(mean[site]["draws"], tot[site]["draws"] / scale)
    unit = run()
    assert np.all(unit[site]["draws"] > 0) and np.all(unit[site]["draws"] < 1)          # an average probability
    # the default grid: 25 points between the column's smallest and largest value
    col = (data["site_covs"] if side == "site" else data["obs_covs"])[..., 0]
    grid = response_curves(models.occu, posterior, **data, side=side, probs=PROBS, **opts)
    assert _same(grid["values"], np.linspace(float(col.min()), float(col.max()), 25).astype(np.float32)) and grid[site]["draws"].shape == (3, 25, 1)


def test_two_species():
    data, posterior, opts = _case("occu", 40, S=2, Ko=2)
    w = np.random.default_rng(42).uniform(0.5, 2.0, 70)
    for side in ("site", "obs"):
        run = lambda post: response_curves(models.occu, post, **data, side=side, covariate=1, values=[-1.0, 0.0, 1.0], weights=w, probs=PROBS)
        both = run(posterior)
        assert both["psi" if side == "site" else "prob_detection"]["draws"].shape == (3, 3, 2)   # the plate is last
        for sp in range(2):
            one = run(_Posterior({key: a[:, sp:sp + 1] for key, a in posterior.sites.items()}))
            for key in ("draws", "mean", "sd", "quantiles"):
                site = curve_name("occu", side)
                assert _same(np.ascontiguousarray(both[site][key][..., sp:sp + 1]), one[site][key]), (side, sp, key)


def test_a_small_fit():
    with contextlib.redirect_stdout(io.StringIO()):
        data, _ = simulate(n_sites=60, random_seed=1)
    res = fit(models.occu, **data, num_chains=1, num_samples=100, num_warmup=100, timeout=600)
    new = {key: f32(data[key]) for key in ("site_covs", "obs_covs")}
    for side in ("site", "obs"):
        got = _contract("occu", new, res.mcmc, {}, side, 0, np.linspace(-2.0, 2.0, 5), None, f"fit {side}")
        site = curve_name("occu", side)
        q = got[site]["quantiles"]
        assert got["n_draws"] == 100 and np.isfinite(q).all() and np.all(q[0] <= q[1]) and np.all(q[1] <= q[2]) and np.all(q > 0) and np.all(q < 1)
        # a logit-linear response is monotone in the covariate, draw by draw
        steps = np.sign(np.diff(got[site]["draws"][..., 0], axis=1))
        assert np.all(steps == steps[:, :1])


def test_the_definition_against_the_float64_logistic_formula():
    """occu, both sides, at the tolerance tests/test_gpu_predict.py holds ``psi`` to (rtol 2e-5, atol 2e-6): an average of terms that
    each meet it meets it."""
    data, posterior, opts = _case("occu", 80, N=101, T=2, J=2, n=5, Ks=3, Ko=2)
    beta, alpha = posterior.sites["beta"][:, 0].astype(np.float64), posterior.sites["alpha"][:, 0].astype(np.float64)
    values = f32([-2.0, -0.3, 1.4])
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    got = response_curves(models.occu, posterior, **data, side="site", covariate=2, values=values, probs=PROBS)
    X = np.repeat(data["site_covs"].astype(np.float64)[None], 3, axis=0)                          # (V, N, Ks)
    X[:, :, 2] = values[:, None]
    want = sig(beta[:, None, None, 0] + np.einsum("vik,nk->nvi", X, beta[:, 1:])).mean(axis=2)    # (n, V)
    np.testing.assert_allclose(got["psi"]["draws"][..., 0], want, rtol=2e-5, atol=2e-6)
    got = response_curves(models.occu, posterior, **data, side="obs", covariate=0, values=values, probs=PROBS)
    W = np.repeat(data["obs_covs"].astype(np.float64)[None], 3, axis=0)                           # (V, N, T, J, Ko)
    W[..., 0] = values[:, None, None, None]
    want = sig(alpha[:, None, None, None, None, 0] + np.einsum("vitjk,nk->nvitj", W, alpha[:, 1:])).mean(axis=(2, 3, 4))
    np.testing.assert_allclose(got["prob_detection"]["draws"][..., 0], want, rtol=2e-5, atol=2e-6)


# ------------------------------------------------------------------------------------------ the C-ABI's refusals ----
def _abi(ds, draws, side, k, values, weight=None, out=True, n_values=None):
    """bl_response_curves through ctypes; the output stays untouched (-7) on a refusal."""
    n = draws.shape[0]
    v = np.ascontiguousarray(values, dtype=np.float32)
    total = np.full((n, max(v.size, 1)), -7.0)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    rc = ds._lib.bl_response_curves(ds._h, n, draws.ctypes.data_as(C.POINTER(C.c_float)), side, k, v.size if n_values is None else n_values,
                                    v.ctypes.data_as(C.POINTER(C.c_float)), dp(weight), dp(total) if out else None)
    return rc, total


def test_refusals_at_the_abi():
    rng = np.random.default_rng(0)
    X, W = f32(rng.normal(size=(20, 1))), f32(rng.normal(size=(20, 2, 2, 1)))
    Y = f32(rng.random((1, 20, 2, 2)) < 0.4)
    blank = lambda J: np.full((1, 20, 2, J), np.nan, dtype=np.float32)
    refused = {"occu_dyn": OccuDataset(X, W, Y, model="occu_dyn"),
               "occu_comb": OccuDataset(X, W, blank(2), model="occu_comb", ARU_obs_covs=rng.normal(size=(20, 2, 3, 1)), ARU_obs=blank(3),
                                        scores_obs=blank(2)),
               "a joint-species handle": OccuDataset(X, W, np.concatenate([Y, Y]))}
    for name, ds in refused.items():
        dr = np.zeros((2, ds.D), dtype=np.float32)
        for side in (0, 1):
            rc, out = _abi(ds, dr, side, 0, [0.5])
            assert rc == _ffi.BL_ERR_UNSUPPORTED and b"bl_response_curves: not built for " + name.encode() in ds._lib.bl_last_error(), name
            assert (out == -7.0).all(), name
        with pytest.raises(NotImplementedError):
            ds.response_curves(dr, 0, 0, [0.5])
        ds.close()
    for name in ("occu_comb", "occu_dyn"):
        with pytest.raises(NotImplementedError, match=name):
            response_curves(getattr(models, name), _Posterior({}), site_covs=X, obs_covs=W)

    ds = OccuDataset(X, W, Y)
    dr = np.zeros((3, ds.D), dtype=np.float32)
    last = ds._lib.bl_last_error
    ok = [0.5, -0.5]
    for side in (2, -1):
        rc, out = _abi(ds, dr, side, 0, ok)
        assert rc == _ffi.BL_ERR_INVALID and b"side=%d" % side in last() and (out == -7.0).all(), side
    for side, k, which in ((0, 1, b"Ks"), (0, -1, b"Ks"), (1, 1, b"Ko"), (1, -3, b"Ko")):
        rc, out = _abi(ds, dr, side, k, ok)
        assert rc == _ffi.BL_ERR_INVALID and b"covariate=%d outside 0 .. %s - 1 = 0" % (k, which) in last() and (out == -7.0).all(), (side, k)
    for bad in (0, -4):
        rc, out = _abi(ds, dr, 0, 0, ok, n_values=bad)
        assert rc == _ffi.BL_ERR_INVALID and b"n_values=%d" % bad in last() and (out == -7.0).all(), bad
    for bad, text in ((np.nan, b"nan"), (np.inf, b"inf"), (-np.inf, b"-inf")):
        rc, out = _abi(ds, dr, 0, 0, [0.5, bad])
        assert rc == _ffi.BL_ERR_INVALID and b"values[1]=" + text + b" is not finite" in last() and (out == -7.0).all(), bad
        w = np.ones(20)
        w[4] = bad
        rc, out = _abi(ds, dr, 1, 0, ok, weight=w)
        assert rc == _ffi.BL_ERR_INVALID and b"weight[4]=" + text + b" is not finite" in last() and (out == -7.0).all(), bad
    rc, out = _abi(ds, dr, 0, 0, ok, out=False)
    assert rc == _ffi.BL_ERR_INVALID and b"curve_total is NULL" in last()
    with pytest.raises(ValueError):
        ds.response_curves(dr, 0, 0, ok, weight=np.ones(5))
    with pytest.raises(ValueError):
        ds.response_curves(dr, 0, 0, [])
    with pytest.raises(ValueError):
        ds.response_curves(dr, 0, 3, ok)
    # a side without covariates: every covariate is outside
    bare = OccuDataset(np.zeros((20, 0), dtype=np.float32), W, Y)
    rc, out = _abi(bare, np.zeros((3, bare.D), dtype=np.float32), 0, 0, ok)
    assert rc == _ffi.BL_ERR_INVALID and b"covariate=0 outside 0 .. Ks - 1 = -1" in last() and (out == -7.0).all()
    rc, out = _abi(bare, np.zeros((3, bare.D), dtype=np.float32), 1, 0, ok)
    assert rc == 0 and not (out == -7.0).any()                  # its obs side is served
    bare.close()
    # a NUTS launch in flight
    ds.launch(num_warmup=200000, num_samples=200000, num_chains=2, seed=0)
    rc, out = _abi(ds, dr, 0, 0, ok)
    assert rc == _ffi.BL_ERR_BUSY and b"in flight" in last() and (out == -7.0).all()
    ds.abort()
    with pytest.raises(Exception, match="aborted"):
        ds.wait()
    rc, out = _abi(ds, dr, 0, 0, ok)
    assert rc == 0 and not (out == -7.0).any()                  # the handle stays usable
    ds.close()
