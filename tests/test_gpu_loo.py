"""PSIS-LOO on the GPU: bl_psis_loo against the float64 restatement of its definition (tests/psis_ref.py), column by column, over the
draw counts at which the definition or the kernel takes another path (no tail to fit below 25 draws; fewer draws than lanes; a partial
last 64-draw strip; the cap) and over cell counts around the transpose's 32-cell tile; ties, constants, ratios at the log(DBL_MIN)
floor and non-finite columns; independence of the launch geometry, bit for bit; the refusals at the C-ABI; and two small fits through
``loo_marginal`` / ``compare_marginal``.

Inputs are hand-made float32 matrices: normal(-3, 0.3) scaled per column by uniform(0.5, 2); every fourth column is -log of exact Pareto
ratios with k0 = 0.7, so that k-hat above 0.5 is exercised.

Tolerances.  Both sides are float64 on bit-equal float32 inputs; what remains is libm (exp, log, log1p, expm1: a few ulp), contraction of
a multiply-add where the source writes one, and the order of sums of at most 8192 terms.  The errors are measured on the scale
1 + |want|.  Largest values observed on the first run on one MI355X, over every case of this
file: k 4.416e-15 (n = 100, 257 cells), elpd 5.463e-16 (n = 1000), lppd 3.549e-16 (n = 1000).  The bounds are 100 x those: k 4.5e-13,
elpd 5.5e-14, lppd 3.6e-14 -- k is the loosest because it is a mean of log1p terms at a b that is itself a weighted mean of 30 to 46
candidates.  Where the restatement says k = inf the device says inf exactly.
No bound may exceed 1e-8 (1 + |want|), whatever is observed (asserted below)."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest

import psis_ref
from biolith_amd import _ffi
from biolith_amd.engine import psis_loo
from biolith_amd.evaluation import lppd_marginal
from biolith_amd.models import occu, occu_rn, simulate
from biolith_amd.utils import compare_marginal, conditional_abundance, conditional_occupancy, fit, loo_marginal

pytestmark = pytest.mark.gpu

# bounds on |got - want| / (1 + |want|): 100 x the largest value observed on the first GPU run (the module's docstring)
BOUND_K, BOUND_ELPD, BOUND_LPPD = 4.5e-13, 5.5e-14, 3.6e-14
assert max(BOUND_K, BOUND_ELPD, BOUND_LPPD) <= 1e-8

_worst = {"k": 0.0, "elpd": 0.0, "lppd": 0.0}


def _matrix(seed, n, cells):
    rng = np.random.default_rng(seed)
    ll = (rng.normal(-3.0, 0.3, (n, cells)) * rng.uniform(0.5, 2.0, cells)).astype(np.float32)
    heavy = np.arange(cells) % 4 == 3
    ll[:, heavy] = (0.7 * np.log1p(-rng.uniform(size=(n, int(heavy.sum())))) - 3.0).astype(np.float32)
    return ll


def _check(ll, got, label):
    """got = (elpd, k, lppd) of the device against the restatement, column by column; prints the largest errors."""
    want = psis_ref.matrix(ll)
    (ge, gk, gl), (we, wk, wl) = got, want
    bad = np.isnan(we)
    for g in got:
        assert np.array_equal(np.isnan(g), bad), label
    assert np.array_equal(np.isinf(gk), np.isinf(wk)) and np.all(gk[np.isinf(wk)] == np.inf), (label, gk, wk)
    fin = np.isfinite(wk)
    err = lambda g, w: float(np.max(np.abs(g - w) / (1.0 + np.abs(w)), initial=0.0))
    ek, ee, el = err(gk[fin], wk[fin]), err(ge[~bad], we[~bad]), err(gl[~bad], wl[~bad])
    for key, v in (("k", ek), ("elpd", ee), ("lppd", el)):
        _worst[key] = max(_worst[key], v)
    print(f"\n[psis_loo {label}] max scaled error: k {ek:.3e} ({int(fin.sum())} finite, max {np.max(wk[fin], initial=-np.inf):.2f}), "
          f"elpd {ee:.3e}, lppd {el:.3e}; so far k {_worst['k']:.3e}, elpd {_worst['elpd']:.3e}, lppd {_worst['lppd']:.3e}")
    assert ek <= BOUND_K and ee <= BOUND_ELPD and el <= BOUND_LPPD, (label, ek, ee, el)
    return want


@pytest.mark.parametrize("n,cells", [(2, 5), (4, 63), (16, 4), (20, 257), (25, 257), (25, 1), (64, 1), (100, 5), (100, 63), (1000, 257),
                                     (4096, 3), (8192, 3)])
def test_against_the_restatement(n, cells):
    ll = _matrix(1000 * n + cells, n, cells)
    if cells >= 4:
        ll[:, 3] = (0.7 * np.log1p(-np.random.default_rng(n).uniform(size=n)) - 3.0).astype(np.float32)
    want = _check(ll, psis_loo(ll), f"n={n} cells={cells}")
    if n < 25:
        assert np.all(want[1] == np.inf)       # M = ceil(n / 5) <= 4: no tail to fit
    else:
        assert np.all(np.isfinite(want[1]))
    if n >= 1000 and cells >= 4:
        assert want[1].max() > 0.5


def _edge_columns(n=4000):
    rng = np.random.default_rng(7)
    base = _matrix(7, n, 12)
    ties = base[:, 1].copy()
    ties[rng.permutation(n)[:3000]] = np.float32(-1.5)           # 3000 equal values, the largest: a finite k from the rest
    low_ties = base[:, 2].copy()
    low_ties[rng.permutation(n)[:3000]] = np.float32(-9.0)       # 3000 equal values, the smallest: all of them at lr = 0, no tail
    base[:, 1], base[:, 2] = ties, low_ties
    base[:, 4] = np.float32(-2.5)                                  # constant
    base[:, 5] = rng.normal(-80.0, 0.3, n).astype(np.float32)     # ll around -80
    base[:, 6] = rng.uniform(-800.0, -80.0, n).astype(np.float32)  # ratios down to and below the log(DBL_MIN) floor
    base[:, 7] = np.float32(-80.0)
    base[17, 7] = np.float32(-800.0)                               # every draw but one below the floor
    return base


def test_ties_constants_and_the_floor():
    ll = _edge_columns()
    want = _check(ll, psis_loo(ll), "edge columns")
    assert np.isfinite(want[1][1]) and want[1][2] == np.inf and want[1][4] == np.inf and want[1][7] == np.inf
    assert abs(want[0][4] + 2.5) < 1e-12


def test_non_finite_columns_are_nan_and_poison_nothing():
    ll = _edge_columns()
    clean = [np.array(a) for a in psis_loo(ll)]
    dirty = ll.copy()
    dirty[5, 3], dirty[3999, 8], dirty[0, 9] = np.nan, -np.inf, np.inf
    got = psis_loo(dirty)
    _check(dirty, got, "non-finite columns")
    bad = np.zeros(ll.shape[1], dtype=bool)
    bad[[3, 8, 9]] = True
    for g, c in zip(got, clean):
        assert np.all(np.isnan(g[bad]))
        assert g[~bad].tobytes() == c[~bad].tobytes()


@pytest.fixture(scope="module")
def wide():
    ll = _matrix(11, 100, 257)
    return ll, [np.array(a) for a in psis_loo(ll)]


def test_geometry_independence(wide):
    ll, ref = wide
    _check(ll, ref, "n=100 cells=257 (the geometry tests' matrix)")
    same = lambda got, cols=slice(None): all(np.asarray(g).tobytes() == r[cols].tobytes() for g, r in zip(got, ref))
    assert same(psis_loo(ll))                                   # the same call twice
    for per in (1, 5, 64, 10 ** 9):
        assert same(psis_loo(ll, cells_per_launch=per)), per    # a chunk boundary at a test's size
    rng = np.random.default_rng(0)
    for cols in (np.array([0]), np.array([256]), np.arange(31, 34), np.sort(rng.permutation(257)[:70])):
        assert same(psis_loo(ll[:, cols]), cols), cols          # any subset of the columns in a call of its own
    assert same(psis_loo(ll.reshape(100, 1, 257, 1)))           # trailing axes fold into the cells
    assert psis_loo(ll.reshape(100, 1, 257, 1))[0].shape == (1, 257, 1)


def _raw(ll, n=None, cells=None, outs=(True, True, True), null_matrix=False, per=0):
    """One call at the C-ABI with sentinel-filled outputs: (rc, message, outputs)."""
    lib = _ffi.load()
    bufs = [np.full(ll.shape[1], -7.0) if o else None for o in outs]
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None
    fp = None if null_matrix else ll.ctypes.data_as(C.POINTER(C.c_float))
    rc = lib.bl_psis_loo(0, ll.shape[0] if n is None else n, ll.shape[1] if cells is None else cells, fp, per, *map(dp, bufs))
    return rc, lib.bl_last_error().decode(), bufs


def test_each_output_alone(wide):
    ll, ref = wide
    ll = np.ascontiguousarray(ll)
    for i in range(3):
        rc, _, bufs = _raw(ll, outs=tuple(j == i for j in range(3)), per=40)
        assert rc == _ffi.BL_OK and bufs[i].tobytes() == ref[i].tobytes()


def test_refusals_at_the_abi():
    """Argument checks, all of them before any launch; the outputs keep their sentinel."""
    ll = np.ascontiguousarray(_matrix(3, 8, 6))
    untouched = lambda bufs: all(b is None or np.all(b == -7.0) for b in bufs)
    rc, msg, bufs = _raw(ll, n=1)
    assert rc == _ffi.BL_ERR_INVALID and "n_draws=1" in msg and untouched(bufs)
    rc, msg, bufs = _raw(ll, outs=(False, False, False))
    assert rc == _ffi.BL_ERR_INVALID and "every output is NULL" in msg
    rc, msg, bufs = _raw(ll, null_matrix=True)
    assert rc == _ffi.BL_ERR_INVALID and "log_lik is NULL" in msg and untouched(bufs)
    rc, msg, bufs = _raw(ll, cells=-1)
    assert rc == _ffi.BL_ERR_INVALID and "cells=-1" in msg and untouched(bufs)
    rc, msg, bufs = _raw(ll, cells=0)
    assert rc == _ffi.BL_OK and untouched(bufs)
    big = np.zeros((_ffi.PSIS_MAX_DRAWS + 1, 2), dtype=np.float32)
    rc, msg, bufs = _raw(big)
    assert rc == _ffi.BL_ERR_UNSUPPORTED and f"BL_PSIS_MAX_DRAWS={_ffi.PSIS_MAX_DRAWS}" in msg and untouched(bufs)
    with pytest.raises(NotImplementedError, match="BL_PSIS_MAX_DRAWS"):
        psis_loo(big)
    with pytest.raises(ValueError, match="n_draws=1"):
        psis_loo(ll[:1])
    assert all(a.shape == (0,) for a in psis_loo(ll[:, :0]))


def test_end_to_end_occu_and_occu_rn():
    with contextlib.redirect_stdout(io.StringIO()):
        data, _ = simulate(n_sites=60)
    kw = dict(num_chains=1, num_warmup=100, num_samples=100, timeout=600)
    lats = {"occu": conditional_occupancy(occu, fit(occu, **data, **kw).mcmc, **data),
            "occu_rn": conditional_abundance(occu_rn, fit(occu_rn, **data, **kw).mcmc, **data)}
    res = {}
    for name, lat in lats.items():
        r = res[name] = loo_marginal(lat, pointwise=True)
        print(f"\n[loo {name}] elpd_loo {r['elpd_loo']:.3f} (se {r['se']:.3f}), p_loo {r['p_loo']:.3f}, k max {r['pareto_k_max']:.3f}, "
              f"{r['n_k_above_0.7']} of {r['n_cells']} cells above 0.7")
        assert all(np.isfinite(r[key]) for key in ("elpd_loo", "p_loo", "looic", "se", "lppd"))
        assert r["p_loo"] > 0 and r["n_draws"] == 100
        assert r["n_cells"] == int((np.asarray(lat["n_obs"]) > 0).sum())
        assert r["lppd"] == pytest.approx(lppd_marginal(lat), rel=1e-10)
        assert r["elpd_loo_i"].shape == np.asarray(lat["n_obs"]).shape
        assert np.array_equal(np.isnan(r["elpd_loo_i"]), np.asarray(lat["n_obs"]) == 0)
    rows = compare_marginal(res)
    assert sorted(r["name"] for r in rows) == ["occu", "occu_rn"]
    assert rows[0]["elpd_loo"] >= rows[1]["elpd_loo"] and rows[0]["elpd_diff"] == 0.0
    assert rows[1]["elpd_diff"] == pytest.approx(rows[1]["elpd_loo"] - rows[0]["elpd_loo"]) and rows[1]["elpd_diff"] <= 0
    assert rows[1]["se_diff"] > 0
