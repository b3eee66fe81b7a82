"""bl_score_posterior on the device against the float64 restatement in tests/scores_ref.py: per-cell and per-visit parity at random
theta, the exact structure (empty cells, masked visits), the sum identity with the sampler's own density on the same handle, the joint
draws and their frequencies across a chunk boundary, the refusals, and fit -> conditional_scores end to end.

Bounds (tests/scores_ref.py: bounds): |l32 - l64| <= rtol S + ulp32(l64) / 2 with S the sum of the absolute values of the cell's terms
and rtol = 2e-6, the occu_cs family's committed bl_logp_grad bound (test_gpu_cs.py); |q32 - q64| <= (bound on A + bound on B) / 4 +
2^-23; f_prob: the same with the visit's three terms (log p_j, n1_j, mix_j) added to A's.  Every check prints the largest measured error
as a fraction of its bound (pytest -s).
The largest measured errors have not been recorded here yet: no run of this module on an MI355X has been made.
"""
import contextlib
import ctypes as C
import io
import math
import time

import numpy as np
import pytest
from scipy import stats

import scores_ref as R
from biolith_amd import _ffi
from biolith_amd.engine import OccuDataset
from biolith_amd.evaluation import expected_true_positives, finite_sample_occupancy, waic_marginal
from biolith_amd.models import occu_cs, simulate_cs
from biolith_amd.models._generators import Generator, expit, within
from biolith_amd.utils import conditional_scores, fit, predict
from conftest import quiet_simulate

pytestmark = pytest.mark.gpu

RTOL = 2e-6   # tests/test_gpu_cs.py: test_cs_logp_grad_parity


def _simulate_cs(**kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return simulate_cs(**kw)


def _log_prior(t, Ks, Ko):
    """The handle's default priors in the engine's coordinates: Normal(0, 1) coefficients; mu0 ~ Normal(0, 10); mu1 ~ Normal(0, 10)
    truncated below at mu0, in x1 = log(mu1 - mu0); sigma_f ~ Gamma(5, 1) in log sigma_f."""
    beta, alpha, mu0, mu1, sg0, sg1 = R.split(t, Ks, Ko)
    lp = float(np.sum(stats.norm.logpdf(np.r_[beta, alpha])))
    lp += float(stats.norm.logpdf(mu0, 0.0, 10.0))
    lp += float(stats.norm.logpdf(mu1, 0.0, 10.0) - stats.norm.logsf(mu0 / 10.0) + math.log(mu1 - mu0))
    for sg in (sg0, sg1):
        lp += float(stats.gamma.logpdf(sg, 5.0, scale=1.0) + math.log(sg))
    return lp


def _thetas(rng, D, n=4):
    """theta ~ U(-2, 2), the score coordinates near the simulator's truth (mu0 = 0, mu1 = 10, sigma0 = 10, sigma1 = 5)."""
    th = rng.uniform(-2, 2, size=(n, D))
    th[:, -4:] = np.array([0.0, math.log(10.0), math.log(10.0), math.log(5.0)]) + rng.uniform(-0.3, 0.3, size=(n, 4))
    return th.astype(np.float32).astype(np.float64)


class Case:
    """One data set, its handle's outputs at four thetas and the restatement's cells: made once, read by the tests below."""

    def __init__(self, seed, **kw):
        data, _ = _simulate_cs(simulate_missing=True, random_seed=seed, **kw)
        self.X, self.W, self.Sc = data["site_covs"], data["obs_covs"], data["obs"][0]
        self.ds = OccuDataset(self.X, self.W, data["obs"], model="occu_cs")
        self.th = _thetas(np.random.default_rng(seed + 20), self.ds.D)
        self.out = self.ds.score_posterior(self.th, seed=5)
        self.U = self.ds.logp_grad(self.th)[0]
        self.cells = [R.cs_cells(self.X, self.W, self.Sc, t) for t in self.th]


@pytest.fixture(scope="module")
def cases():
    made = {"N70_T2_J5": Case(1, n_sites=70, n_periods=2, deployment_days_per_site=35, n_site_covs=2, n_obs_covs=2),
            "N300_T1_J1": Case(2, n_sites=300, n_periods=1, deployment_days_per_site=7, n_site_covs=1, n_obs_covs=1)}
    yield made
    for c in made.values():
        c.ds.close()


@pytest.mark.parametrize("name", ["N70_T2_J5", "N300_T1_J1"])
def test_parity(cases, name):
    c = cases[name]
    ds, th = c.ds, c.th
    ll, q, z, fp, f = c.out
    n, T, N, J = th.shape[0], ds.T, ds.N, ds.J
    assert (N, T, J) == {"N70_T2_J5": (70, 2, 5), "N300_T1_J1": (300, 1, 1)}[name]
    assert ll.shape == q.shape == z.shape == (n, T, N) and fp.shape == f.shape == (n, J, T, N)
    assert ll.dtype == q.dtype == fp.dtype == np.float32 and z.dtype == f.dtype == np.uint8
    assert np.all(np.isfinite(ll)) and np.all(np.isfinite(fp))
    worst = dict(l=0.0, q=0.0, f=0.0, s=0.0)
    for b in range(n):
        r = c.cells[b]
        bl, bq, bf = R.bounds(r, RTOL)
        el, eq, ef = np.abs(ll[b] - r["l"]), np.abs(q[b] - r["q"]), np.abs(fp[b] - r["f_prob"])
        worst["l"], worst["q"], worst["f"] = max(worst["l"], float(np.max(el / bl))), max(worst["q"], float(np.max(eq / bq))), max(worst["f"], float(np.max(ef / bf)))
        assert np.all(el <= bl), (name, b, float(np.max(el / bl)))
        assert np.all(eq <= bq), (name, b, float(np.max(eq / bq)))
        assert np.all(ef <= bf), (name, b, float(np.max(ef / bf)))
        empty = r["n_obs"] == 0
        assert empty.any() and np.all(ll[b][empty] == 0.0)                    # exactly: nothing observed, likelihood 1
        assert np.all(np.abs(q[b][empty] - r["psi"][empty]) <= bq[empty])     # ... and the conditional is the prior
        masked = ~r["m"]
        assert masked.any() and (J == 1 or (masked & ~empty[None]).any())     # J > 1: masked visits in cells that do have data
        want_masked = (r["q"][None] * r["p"])[masked]                         # no score to condition on: f_prob = z_prob p_j
        assert np.all(np.abs(fp[b][masked] - want_masked) <= bf[masked])
        # the new kernel's cells add up to the likelihood part of the sampler's own potential
        want, got = -c.U[b] - _log_prior(th[b], ds.Ks, ds.Ko), float(ll[b].astype(np.float64).sum())
        worst["s"] = max(worst["s"], abs(got - want) / (RTOL * abs(want)))
        assert abs(got - want) <= RTOL * abs(want), (name, b, got, want)
    print(f"\n[{name}] max error / bound: log_lik {worst['l']:.3f}, z_prob {worst['q']:.3f}, f_prob {worst['f']:.3f}, sum identity {worst['s']:.3f}")


def test_invariants_seeds_and_split_calls(cases):
    c = cases["N70_T2_J5"]
    ds, th = c.ds, c.th
    ll, q, z, fp, f = c.out
    assert np.all((0 <= fp) & (fp <= q[:, None]) & (q[:, None] <= 1))
    assert set(np.unique(z)) <= {0, 1} and set(np.unique(f)) <= {0, 1} and np.all(f <= z[:, None])
    assert 0 < z.mean() < 1 and 0 < f.mean() < 1
    same, other = ds.score_posterior(th, seed=5), ds.score_posterior(th, seed=6)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(c.out, same))
    assert other[2].tobytes() != z.tobytes() and other[4].tobytes() != f.tobytes()
    assert other[0].tobytes() == ll.tobytes() and other[3].tobytes() == fp.tobytes()
    # z does not depend on whether the visit level is asked for (conditional_scores makes the two calls)
    cells_only = ds.score_posterior(th, seed=5, visits=False)
    assert cells_only[3] is None and cells_only[4] is None and all(a.tobytes() == b.tobytes() for a, b in zip(c.out[:3], cells_only[:3]))
    # split at an odd index: the first call's outputs are the one call's, byte for byte, the draws included.  The entry numbers a
    # call's draws from 0 (it has no offset argument), so the second call's z and f belong to other generator keys; what does not
    # depend on the key is again byte-identical.  (Draw numbers that are not a chunk's own: test_draw_frequencies_across_a_chunk_boundary.)
    head, tail = ds.score_posterior(th[:3], seed=5), ds.score_posterior(th[3:], seed=5)
    assert all(a.tobytes() == b[:3].tobytes() for a, b in zip(head, c.out))
    assert all(tail[k].tobytes() == c.out[k][3:].tobytes() for k in (0, 1, 3))
    assert np.all(tail[4] <= tail[2][:, None])


def test_draw_frequencies_across_a_chunk_boundary():
    X, W, Sc, th, n = R.frequency_case()
    r = R.cs_cells(X, W, Sc, th)
    ds = OccuDataset(X, W, Sc[None], model="occu_cs")
    ll, q, z, fp, f = ds.score_posterior(np.tile(th.astype(np.float32), (n, 1)), seed=3)
    ds.close()
    per_draw = fp[0].nbytes
    first = (256 << 20) // per_draw                   # the draws of the first 256 MB chunk of device scratch
    assert fp.nbytes > (256 << 20) and 0 < first < n - 1
    for a in (ll, q, fp):                             # one theta: every draw's deterministic outputs are draw 0's, on both sides
        assert np.all(a[first - 1] == a[0]) and np.all(a[first] == a[0]) and np.all(a[-1] == a[0])
    bl, bq, bf = R.bounds(r, RTOL)
    assert np.all(np.abs(ll[-1] - r["l"]) <= bl) and np.all(np.abs(q[-1] - r["q"]) <= bq) and np.all(np.abs(fp[-1] - r["f_prob"]) <= bf)
    # the generator's key is the absolute draw number: the second chunk does not replay the first one's uniforms
    assert z[first:].tobytes() != z[:n - first].tobytes() and f[first:].tobytes() != f[:n - first].tobytes()
    assert np.all(f <= z[:, None])
    # z against the kernel's own z_prob, f against its own f_prob, each pooled with the variance the model gives the sum (the f of a
    # cell share its z: tests/scores_ref.py: pooled_statistics); the restatement alone meets the same criterion (test_scores_cpu.py)
    got = R.pooled_statistics(r, z.sum(axis=0, dtype=np.int64), f.sum(axis=0, dtype=np.int64), n, z_prob=q[0], f_prob=fp[0])
    assert got["z"][1] >= 1000 and got["f"][1] >= 8000, got
    print("\n[draws] " + "; ".join(f"{k}: {cnt} x {n} draws in range, standardised sum {stat:.3f}" for k, (stat, cnt) in got.items()))
    assert abs(got["z"][0]) <= 4.5 and abs(got["f"][0]) <= 4.5, got


def test_abi_refusals_and_busy():
    data, _, _ = quiet_simulate(n_sites=60, deployment_days_per_site=28, random_seed=1)
    X, W, Y = data["site_covs"], data["obs_covs"], data["obs"]
    cnt = np.nan_to_num(Y) * 2
    handles = [("occu", OccuDataset(X, W, Y)), ("occu_rn", OccuDataset(X, W, Y, model="occu_rn", max_abundance=20)),
               ("nmixture", OccuDataset(X, W, cnt, model="nmixture", max_abundance=20)),
               ("occu_cop", OccuDataset(X, W, cnt, model="occu_cop", fp_mode=None, session_duration=np.ones(Y.shape[1:]))),
               ("occu_dyn", OccuDataset(X, W, Y, model="occu_dyn")), ("joint-species", OccuDataset(X, W, np.concatenate([Y, Y])))]
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    for name, ds in handles:
        dr = np.zeros((2, ds.D), dtype=np.float32)
        out = np.zeros((2, ds.T, ds.N), dtype=np.float32)
        assert ds._lib.bl_score_posterior(ds._h, 2, fp(dr), 0, fp(out), None, None, None, None) == _ffi.BL_ERR_UNSUPPORTED, name
        assert name in ds._lib.bl_last_error().decode(), (name, ds._lib.bl_last_error())
        with pytest.raises(NotImplementedError):
            ds.score_posterior(dr)
        ds.close()
    scores = np.where(np.isnan(Y), np.nan, Y * 10.0 - 1.0)
    ds = OccuDataset(X, W, scores, model="occu_cs")
    dr = np.zeros((2, ds.D), dtype=np.float32)
    assert ds._lib.bl_score_posterior(ds._h, 2, fp(dr), 0, None, None, None, None, None) == _ffi.BL_ERR_INVALID
    assert ds._lib.bl_score_posterior(ds._h, 0, None, 0, None, None, None, None, None) == _ffi.BL_ERR_INVALID
    only_f = np.zeros((2, ds.J, ds.T, ds.N), dtype=np.uint8)   # any single output alone is served
    assert ds._lib.bl_score_posterior(ds._h, 2, fp(dr), 0, None, None, None, None, only_f.ctypes.data_as(C.POINTER(C.c_uint8))) == _ffi.BL_OK
    # the other three conditionals still refuse this handle
    for entry in (ds.site_posterior, ds.abundance_posterior, ds.path_posterior):
        with pytest.raises(NotImplementedError, match="occu_cs"):
            entry(dr)
    ds.close()
    big, _ = _simulate_cs(n_sites=2000, n_site_covs=2, n_obs_covs=2, deployment_days_per_site=140)
    db = OccuDataset(big["site_covs"], big["obs_covs"], big["obs"], model="occu_cs")
    db.launch(num_warmup=200000, num_samples=200000, num_chains=2, seed=0)
    time.sleep(0.2)
    assert not db.done()
    one = np.zeros((1, db.D), dtype=np.float32)
    with pytest.raises(_ffi.EngineError) as ei:
        db.score_posterior(one)
    assert ei.value.code == _ffi.BL_ERR_BUSY
    db.abort()
    with pytest.raises(Exception, match="aborted"):
        db.wait()
    assert db.score_posterior(one)[3].shape == (1, db.J, db.T, db.N)   # the handle stays usable
    db.close()


def _simulate_cs_with_f(n_sites, random_seed=0):
    """simulate_cs's defaults (models/occu_cs.py) with the indicator f it draws and drops kept: the same callbacks on the same
    generator, so the same stream -- the caller checks the scores against simulate_cs's own."""
    mu0, sigma0, mu1, sigma1 = 0, 10, 10, 5
    n_replicates, kept = round(365 / 7), {}

    def latent(rng, occ_linear):
        return rng.binomial(n=1, p=expit(occ_linear)[:, None, :], size=(1, 1, n_sites))

    def observe(rng, det_linear, z_site, _):
        shape = (1, n_sites, 1, n_replicates)
        f = rng.binomial(n=1, p=expit(det_linear) * z_site[..., None], size=shape)
        kept["f"] = f
        return rng.normal(loc=np.where(f == 1, mu1, mu0), scale=np.where(f == 1, sigma1, sigma0), size=shape)

    d = Generator(1, n_sites, 1, n_replicates, 1, 1, latent, observe, lambda d: within(d.latent.mean(), 0.25, 0.75)).run(random_seed)
    return d.obs, kept["f"]


def _auc(score, truth):
    """P(score of a positive > score of a negative), ties counted half (Mann-Whitney)."""
    rank = stats.rankdata(score)
    n1 = int(truth.sum())
    n0 = truth.size - n1
    return float((rank[truth].sum() - n1 * (n1 + 1) / 2) / (n1 * n0))


def test_end_to_end():
    data, truth = _simulate_cs(n_sites=80)
    scores, f_true = _simulate_cs_with_f(80)
    assert np.array_equal(scores, data["obs"])
    res = fit(occu_cs, **data, num_chains=1, num_warmup=150, num_samples=100)
    lat = conditional_scores(occu_cs, res.mcmc, **data, random_seed=4)
    n, T, N, J = 100, 1, 80, 52
    assert list(lat) == ["psi", "z_prob", "z", "log_lik", "n_obs", "f_prob", "f"]
    for k, dt in (("psi", np.float32), ("z_prob", np.float32), ("z", np.int32), ("log_lik", np.float32)):
        assert lat[k].shape == (n, T, N, 1) and lat[k].dtype == dt, k
    assert lat["n_obs"].shape == (T, N, 1) and lat["n_obs"].dtype == np.int32 and np.all(lat["n_obs"] == J)
    assert lat["f_prob"].shape == lat["f"].shape == (n, J, T, N, 1) and lat["f_prob"].dtype == np.float32 and lat["f"].dtype == np.int32
    assert np.all(lat["f"] <= lat["z"][:, None])      # the second call drew f jointly with the first call's z
    np.testing.assert_allclose(lat["psi"], res.samples["psi"], rtol=2e-6, atol=1e-7)
    zt = np.asarray(truth["z"])[0, 0] == 1            # (S, T, N)
    zq = lat["z_prob"].mean(0)[0, :, 0]
    print(f"\n[cs e2e] mean z_prob: occupied sites {zq[zt].mean():.4f}, unoccupied {zq[~zt].mean():.4f}")
    assert zq[zt].mean() > zq[~zt].mean()
    ft = f_true[0, :, 0, :].T == 1                    # (S, N, T, J) -> (J, N)
    seen = np.isfinite(data["obs"][0, :, 0, :]).T     # the unmasked visits (all of them here: no missingness was simulated)
    preds = predict(occu_cs, res.mcmc, **data, num_samples=n)
    auc_post = _auc(lat["f_prob"].mean(0)[:, 0, :, 0][seen], ft[seen])
    auc_prior = _auc(preds["f"].mean(0)[:, 0, :, 0][seen], ft[seen])
    print(f"[cs e2e] AUC of the true f: posterior-mean f_prob {auc_post:.4f}, predict's prior f {auc_prior:.4f}")
    assert auc_post > auc_prior
    etp = expected_true_positives(lat)
    assert etp.shape == (n, T, N, 1) and np.all(etp <= J * lat["z_prob"].astype(np.float64) * (1 + 1e-6))
    assert finite_sample_occupancy(lat).shape == (n, T, 1)
    assert all(np.isfinite(v) for v in waic_marginal(lat).values())
