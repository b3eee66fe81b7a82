"""bl_count_posterior on the device against the float64 restatement in tests/counts_ref.py: per-cell and per-visit parity at random
theta over the capacities, the three false-positive modes and the random-effects kinds, the sum identity with the sampler's own density
on the same handle, the exact structure (empty cells, masked visits, Poisson(0)), the joint draws and their frequencies across a chunk
boundary, determinism and the optional outputs, the refusals, and fit -> conditional_counts end to end.

Bounds (tests/counts_ref.py: bounds): |l32 - l64| <= rtol S + ulp32(l64) / 2 with S the sum of the absolute values of the cell's terms
and rtol = 2e-6, the occu_cop family's committed bl_logp_grad bound (test_gpu_cop.py, test_gpu_cop_re.py);
|q32 - q64| <= (bound on A + bound on B) / 4 + 2^-23; true_mean: the same with the visit's two terms (nu_j, phi) added to A's, scaled
by y_j.  Every check prints the largest measured error as a fraction of its bound (pytest -s).
The largest measured errors have not been recorded here yet: no run of this module on an MI355X has been made.

The frequency test requires at least 1000 cells and 4500 visits in range, the restatement's own figures (tests/test_counts_cpu.py).
"""
import contextlib
import ctypes as C
import io
import time

import numpy as np
import pytest

import counts_ref as R
from biolith_amd import _ffi
from biolith_amd.engine import OccuDataset
from biolith_amd.evaluation import expected_true_detections, finite_sample_occupancy, waic_marginal
from biolith_amd.models import occu_cop, simulate_comb, simulate_cop
from biolith_amd.utils import conditional_counts, fit
from conftest import quiet_simulate

pytestmark = pytest.mark.gpu

RTOL = 2e-6   # tests/test_gpu_cop.py, tests/test_gpu_cop_re.py: the logp parity of the family
MIN_Z_CELLS, MIN_T_VISITS = 1000, 4500   # tests/test_counts_cpu.py


def _quiet(fn, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(**kw)


def _thetas(rng, N, T, J, Ks, Ko, fp, site, obs, n=4):
    """Coefficients ~ U(-1, 1) (U(-0.35, 0.35) at capacity 16, as tests/test_gpu_latent.py); phi = log rate: one theta at a very small
    rate (-6), one at a large one (1.5), the others U(-2, 0.5); log sds ~ U(-1, 0), effects ~ Normal(0, 0.5)."""
    o = R.L.occu_theta_layout(N, T, J, Ks, Ko, fp, site, obs)
    G = Ks + Ko + 2
    th = rng.normal(scale=0.5, size=(n, o["D"]))
    th[:, :G] = rng.uniform(-1.0, 1.0, size=(n, G)) * (0.35 if max(Ks, Ko) > 8 else 1.0)
    at = G
    if fp:
        th[:, at] = np.r_[-6.0, 1.5, rng.uniform(-2.0, 0.5, size=n - 2)]
        at += 1
    th[:, at:at + int(site) + int(obs)] = rng.uniform(-1.0, 0.0, size=(n, int(site) + int(obs)))
    return th.astype(np.float32).astype(np.float64)


class Case:
    """One data set, its handle's outputs at four thetas and the restatement's cells: made once, read by the tests below."""

    def __init__(self, seed, N, T, Ks, Ko, mode, site=False, obs=False, J=4):
        rng = np.random.default_rng(seed)
        self.X, self.W, self.Y, self.Dur = R.make_data(rng, N, T, J, Ks, Ko)
        self.kw = dict(fp_mode=mode, site_re=site, obs_re=obs)
        re = dict(site_random_effects=site, obs_random_effects=obs) if site or obs else {}
        self.ds = OccuDataset(self.X, self.W, self.Y[None], model="occu_cop", fp_mode=mode, session_duration=self.Dur, **re)
        self.th = _thetas(rng, N, T, J, Ks, Ko, mode is not None, site, obs)
        assert self.ds.D == self.th.shape[1]
        self.out = self.ds.count_posterior(self.th, seed=5)
        self.U = self.ds.logp_grad(self.th)[0]
        self.cells = [R.cop_cells(self.X, self.W, self.Y, self.Dur, t, **self.kw) for t in self.th]
        self.dims = (N, T, J, Ks, Ko)


PLAIN = [(T, Ks, Ko, mode) for T in (1, 3) for Ks, Ko in ((0, 0), (2, 3), (16, 16)) for mode in (None, "constant", "unoccupied")]
RE = [("site", True, False, None), ("obs", False, True, None), ("both", True, True, None), ("both_rate", True, True, "constant")]
_made = {}


def _case(key):
    if key not in _made:
        if key[0] == "re":
            _, name, site, obs, mode = key
            _made[key] = Case(40 + [r[0] for r in RE].index(name), 300, 3, 2, 3, mode, site, obs)
        else:
            T, Ks, Ko, mode = key
            _made[key] = Case(10 + PLAIN.index(key), 150 if T == 1 else 300, T, Ks, Ko, mode)
    return _made[key]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for c in _made.values():
        c.ds.close()
    _made.clear()


def _check_parity(c, name):
    ds, th = c.ds, c.th
    ll, q, z, tm, tc = c.out
    N, T, J, Ks, Ko = c.dims
    n = th.shape[0]
    assert ll.shape == q.shape == z.shape == (n, T, N) and tm.shape == tc.shape == (n, J, T, N)
    assert ll.dtype == q.dtype == tm.dtype == np.float32 and z.dtype == np.uint8 and tc.dtype == np.int32
    assert np.all(np.isfinite(ll)) and np.all(np.isfinite(tm))
    worst = dict(l=0.0, q=0.0, t=0.0, s=0.0)
    for b in range(n):
        r = c.cells[b]
        bl, bq, bt = R.bounds(r, RTOL)
        el, eq, et = np.abs(ll[b] - r["l"]), np.abs(q[b] - r["q"]), np.abs(tm[b] - r["true_mean"])
        pos = bt > 0
        worst["l"], worst["q"] = max(worst["l"], float(np.max(el / bl))), max(worst["q"], float(np.max(eq / bq)))
        worst["t"] = max(worst["t"], float(np.max(et[pos] / bt[pos])))
        assert np.all(el <= bl), (name, b, float(np.max(el / bl)))
        assert np.all(eq <= bq), (name, b, float(np.max(eq / bq)))
        assert np.all(et <= bt), (name, b, float(np.max(et[pos] / bt[pos])))
        # sum identity: the new kernel's cells add up to the likelihood part of the sampler's own potential on the same handle
        want = -c.U[b] - R.log_prior(th[b], N, T, J, Ks, Ko, **c.kw)
        got = float(ll[b].astype(np.float64).sum())
        worst["s"] = max(worst["s"], abs(got - want) / (RTOL * abs(want)))
        assert abs(got - want) <= RTOL * abs(want), (name, b, got, want)
        # exact structure
        empty, masked = r["n_obs"] == 0, ~r["m"]
        assert empty[:, 0].all() and np.all(ll[b][empty] == 0.0)                    # exactly: nothing observed, likelihood 1
        assert np.all(np.abs(q[b][empty] - r["psi"][empty]) <= bq[empty])           # ... and the conditional is the prior
        assert masked.any() and (masked & ~empty[None]).any()
        assert np.all(tm[b][masked] == 0.0) and np.all(tc[b][masked] == 0)          # a masked visit has no count
        assert np.all(tc[b] >= 0) and np.all(tc[b] <= z[b][None].astype(np.int64) * r["y"].astype(np.int64))
        if c.kw["fp_mode"] is None:
            sure = (r["y_sum"] > 0) & ~empty
            assert sure.any() and np.all(q[b][sure] >= 1 - 2.0 ** -24) and np.all(z[b][sure] == 1)   # Poisson(0) met a count
        if c.kw["fp_mode"] != "constant":
            assert np.array_equal(tc[b], z[b][None].astype(np.int32) * r["y"].astype(np.int32))      # rho = 1: every detection of an occupied cell is real
    assert set(np.unique(z)) <= {0, 1}
    print(f"\n[{name}] max error / bound: log_lik {worst['l']:.3f}, z_prob {worst['q']:.3f}, true_mean {worst['t']:.3f}, sum identity {worst['s']:.3f}")


@pytest.mark.parametrize("T,Ks,Ko,mode", PLAIN)
def test_parity(T, Ks, Ko, mode):
    _check_parity(_case((T, Ks, Ko, mode)), f"T{T}_K{Ks}x{Ko}_{mode}")


@pytest.mark.parametrize("name,site,obs,mode", RE)
def test_parity_random_effects(name, site, obs, mode):
    _check_parity(_case(("re", name, site, obs, mode)), "re_" + name)


def test_determinism_and_optional_outputs():
    c = _case((3, 2, 3, "constant"))
    ds, th = c.ds, c.th
    ll, q, z, tm, tc = c.out
    assert 0 < z.mean() < 1 and (tc < z[:, None] * c.cells[0]["y"][None]).any()     # some counted detections were drawn as false
    same, other = ds.count_posterior(th, seed=5), ds.count_posterior(th, seed=6)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(c.out, same))
    assert other[2].tobytes() != z.tobytes() and other[4].tobytes() != tc.tobytes()
    assert other[0].tobytes() == ll.tobytes() and other[1].tobytes() == q.tobytes() and other[3].tobytes() == tm.tobytes()
    # z does not depend on whether the visit level is asked for (conditional_counts makes the two calls)
    cells_only = ds.count_posterior(th, seed=5, visits=False)
    assert cells_only[3] is None and cells_only[4] is None and all(a.tobytes() == b.tobytes() for a, b in zip(c.out[:3], cells_only[:3]))
    # split at an odd index: the head call's outputs are the full call's, byte for byte, the draws included.  The entry numbers a
    # call's draws from 0, so the tail call's z and true_count belong to other generator keys; what does not depend on the key is again
    # byte-identical.
    head, tail = ds.count_posterior(th[:3], seed=5), ds.count_posterior(th[3:], seed=5)
    assert all(a.tobytes() == b[:3].tobytes() for a, b in zip(head, c.out))
    assert all(tail[k].tobytes() == c.out[k][3:].tobytes() for k in (0, 1, 3))
    # each output alone equals its part of the full call
    n = th.shape[0]
    d32 = np.ascontiguousarray(th, dtype=np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    types = (C.c_float, C.c_float, C.c_uint8, C.c_float, C.c_int32)
    for k in range(5):
        alone = np.zeros_like(c.out[k])
        ptrs = [alone.ctypes.data_as(C.POINTER(types[k])) if m == k else None for m in range(5)]
        assert ds._lib.bl_count_posterior(ds._h, n, fp(d32), 5, *ptrs) == _ffi.BL_OK
        assert alone.tobytes() == c.out[k].tobytes(), k


def test_draw_frequencies_across_a_chunk_boundary():
    X, W, Y, Dur, th, n = R.frequency_case()
    r = R.cop_cells(X, W, Y, Dur, th, fp_mode="constant")
    ds = OccuDataset(X, W, Y[None], model="occu_cop", fp_mode="constant", session_duration=Dur)
    ll, q, z, tm, tc = ds.count_posterior(np.tile(th.astype(np.float32), (n, 1)), seed=3)
    ds.close()
    per_draw = tm[0].nbytes
    first = (256 << 20) // per_draw                   # the draws of the first 256 MB chunk of device scratch
    assert tm.nbytes > (256 << 20) and 0 < first < n - 1
    for a in (ll, q, tm):                             # one theta: every draw's deterministic outputs are draw 0's, on both sides
        assert np.all(a[first - 1] == a[0]) and np.all(a[first] == a[0]) and np.all(a[-1] == a[0])
    bl, bq, bt = R.bounds(r, RTOL)
    assert np.all(np.abs(ll[-1] - r["l"]) <= bl) and np.all(np.abs(q[-1] - r["q"]) <= bq) and np.all(np.abs(tm[-1] - r["true_mean"]) <= bt)
    # the generator's key is the absolute draw number: the second chunk does not replay the first one's uniforms
    assert z[first:].tobytes() != z[:n - first].tobytes() and tc[first:].tobytes() != tc[:n - first].tobytes()
    assert np.all(tc <= z[:, None] * r["y"][None].astype(np.int32))
    # z against the kernel's own z_prob, true_count against its own true_mean, each pooled with the variance the model gives the sum
    # (the counts of a cell share its z: tests/counts_ref.py: pooled_statistics); the restatement alone meets the same criterion
    got = R.pooled_statistics(r, z.sum(axis=0, dtype=np.int64), tc.sum(axis=0, dtype=np.int64), n, z_prob=q[0], true_mean=tm[0])
    assert got["z"][1] >= MIN_Z_CELLS and got["t"][1] >= MIN_T_VISITS, got
    print("\n[draws] " + "; ".join(f"{k}: {cnt} x {n} draws in range, standardised sum {stat:.3f}" for k, (stat, cnt) in got.items()))
    assert abs(got["z"][0]) <= 4.5 and abs(got["t"][0]) <= 4.5, got


def test_abi_refusals_and_busy():
    data, _, _ = quiet_simulate(n_sites=60, deployment_days_per_site=28, random_seed=1)
    X, W, Y = data["site_covs"], data["obs_covs"], data["obs"]
    cnt = np.nan_to_num(Y) * 2
    scores = np.where(np.isnan(Y), np.nan, Y * 10.0 - 1.0)
    comb = _quiet(simulate_comb, n_sites=40)
    handles = [("occu", OccuDataset(X, W, Y)), ("occu_fp", OccuDataset(X, W, Y, model="occu_fp", fp_mode="constant")),
               ("occu_re", OccuDataset(X, W, Y, model="occu_re", site_random_effects=True)),
               ("occu_rn", OccuDataset(X, W, Y, model="occu_rn", max_abundance=20)),
               ("nmixture", OccuDataset(X, W, cnt, model="nmixture", max_abundance=20)),
               ("occu_cs", OccuDataset(X, W, scores, model="occu_cs")),
               ("occu_dyn", OccuDataset(X, W, Y, model="occu_dyn")),
               ("occu_comb", OccuDataset(comb[0]["site_covs"], comb[0]["PC_obs_covs"], comb[0]["PC_obs"][:1], model="occu_comb",
                                         ARU_obs_covs=comb[0]["ARU_obs_covs"], ARU_obs=comb[0]["ARU_obs"][:1], scores_obs=comb[0]["scores_obs"][:1])),
               ("joint-species", OccuDataset(X, W, np.concatenate([Y, Y])))]
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    for name, ds in handles:
        dr = np.zeros((2, ds.D), dtype=np.float32)
        out = np.zeros((2, ds.T, ds.N), dtype=np.float32)
        assert ds._lib.bl_count_posterior(ds._h, 2, fp(dr), 0, fp(out), None, None, None, None) == _ffi.BL_ERR_UNSUPPORTED, name
        assert name in ds._lib.bl_last_error().decode(), (name, ds._lib.bl_last_error())
        with pytest.raises(NotImplementedError):
            ds.count_posterior(dr)
        ds.close()
    ds = OccuDataset(X, W, cnt, model="occu_cop", fp_mode=None, session_duration=np.ones(Y.shape[1:]))
    dr = np.zeros((2, ds.D), dtype=np.float32)
    assert ds._lib.bl_count_posterior(ds._h, 2, fp(dr), 0, None, None, None, None, None) == _ffi.BL_ERR_INVALID
    assert ds._lib.bl_count_posterior(ds._h, 0, fp(dr), 0, fp(np.zeros((2, ds.T, ds.N), dtype=np.float32)), None, None, None, None) == _ffi.BL_ERR_INVALID
    assert ds._lib.bl_count_posterior(ds._h, 2, None, 0, fp(np.zeros((2, ds.T, ds.N), dtype=np.float32)), None, None, None, None) == _ffi.BL_ERR_INVALID
    # the four other conditionals still refuse this handle
    for entry in (ds.site_posterior, ds.abundance_posterior, ds.path_posterior, ds.score_posterior):
        with pytest.raises(NotImplementedError, match="occu_cop"):
            entry(dr)
    ds.close()
    big, _ = _quiet(simulate_cop, n_sites=2000, n_site_covs=2, n_obs_covs=2, deployment_days_per_site=140)
    db = OccuDataset(big["site_covs"], big["obs_covs"], big["obs"], model="occu_cop", fp_mode="constant", session_duration=big["session_duration"])
    db.launch(num_warmup=200000, num_samples=200000, num_chains=2, seed=0)
    time.sleep(0.2)
    assert not db.done()
    one = np.zeros((1, db.D), dtype=np.float32)
    with pytest.raises(_ffi.EngineError) as ei:
        db.count_posterior(one)
    assert ei.value.code == _ffi.BL_ERR_BUSY
    db.abort()
    with pytest.raises(Exception, match="aborted"):
        db.wait()
    assert db.count_posterior(one)[3].shape == (1, db.J, db.T, db.N)   # the handle stays usable
    db.close()


def test_end_to_end():
    data, truth = _quiet(simulate_cop, n_sites=100)
    assert data["false_positives_constant"] is True
    res = fit(occu_cop, **data, num_chains=2, num_warmup=300, num_samples=250)
    lat = conditional_counts(occu_cop, res.mcmc, **data, random_seed=4)
    n, T, N, J = 500, 1, 100, 52
    assert list(lat) == ["psi", "z_prob", "z", "log_lik", "n_obs", "true_mean", "true_count"]
    for k, dt in (("psi", np.float32), ("z_prob", np.float32), ("z", np.int32), ("log_lik", np.float32)):
        assert lat[k].shape == (n, T, N, 1) and lat[k].dtype == dt, k
    assert lat["n_obs"].shape == (T, N, 1) and lat["n_obs"].dtype == np.int32 and np.all(lat["n_obs"] == J)
    assert lat["true_mean"].shape == lat["true_count"].shape == (n, J, T, N, 1)
    assert lat["true_mean"].dtype == np.float32 and lat["true_count"].dtype == np.int32
    y = np.asarray(data["obs"])[0].transpose(2, 1, 0)[None, ..., None]                     # (S, N, T, J) -> (1, J, T, N, 1)
    assert np.all(lat["true_count"] <= lat["z"][:, None] * y)        # the second call drew the counts jointly with the first call's z
    np.testing.assert_allclose(lat["psi"], res.samples["psi"], rtol=2e-6, atol=1e-7)
    assert all(np.isfinite(v) for v in waic_marginal(lat).values())
    fs = finite_sample_occupancy(lat)
    assert fs.shape == (n, T, 1)
    print(f"\n[cop e2e] finite-sample occupancy {fs.mean():.4f}, truth {truth['z'].mean():.4f}")
    assert abs(fs.mean() - truth["z"].mean()) <= 0.1                 # the reference's own atol for psi
    etd = expected_true_detections(lat)
    assert etd.shape == (n, T, N, 1) and np.all(etd <= y.sum(axis=1) * (1 + 1e-6))
    # two species, no rate: served species by species (shapes only)
    data2, _ = _quiet(simulate_cop, n_sites=60, n_species=2, deployment_days_per_site=35)
    data2.pop("false_positives_constant")
    res2 = fit(occu_cop, **data2, num_chains=1, num_warmup=50, num_samples=40)
    lat2 = conditional_counts(occu_cop, res2.mcmc, **data2)
    assert lat2["z_prob"].shape == lat2["z"].shape == lat2["log_lik"].shape == (40, 1, 60, 2) and lat2["n_obs"].shape == (1, 60, 2)
    assert lat2["true_mean"].shape == lat2["true_count"].shape == (40, 5, 1, 60, 2)
    assert np.all(lat2["true_count"] == lat2["z"][:, None] * np.asarray(data2["obs"]).transpose(3, 2, 1, 0)[None])
