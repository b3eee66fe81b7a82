"""Conditional dynamics of occu_dyn, everything that needs no device: the float64 restatement (tests/dyn_path_ref.py) against a literal
statement of the model with the 2^T paths summed by brute force and against the oracle's potential; the kernel's arithmetic emulated
in float32 against the bounds the GPU test asserts (so the bounds are known to be reachable before a device is asked); forward
filtering backward sampling checked by a statistic that an independent sampler fails; ``finite_sample_turnover``; the refusals; the
ABI's declaration; and the GPU end-to-end test's inequalities for the reference alone."""
import contextlib
import io
import itertools
import os

import numpy as np
import pytest
from scipy import stats

import dyn_path_ref as R
import oracle
from biolith_amd import _ffi
from biolith_amd.evaluation import finite_sample_turnover
from biolith_amd.models import nmixture, occu, occu_comb, occu_cop, occu_cs, occu_dyn, occu_rn, simulate_dyn
from biolith_amd.utils import conditional_dynamics, conditional_occupancy
from test_dyn_cpu import _data


def _brute(X, W, Y, th):
    """l (N,), q (T, N), col, ext (T - 1, N) from the model as written: every path z in {0, 1}^T weighed by p(z) p(y | z)."""
    X32, W32, Y32 = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (X, W, Y))
    N, T, J, Ko = W32.shape
    B = X32.shape[1] + 1
    mask = np.isfinite(Y32) & ~np.isnan(W32).any(-1) & ~np.isnan(X32).any(-1)[:, None, None]
    Xc, Wc = np.nan_to_num(X32), np.nan_to_num(W32)
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))  # noqa: E731
    psi, gam, eps = (sig(th[b * B] + Xc @ th[b * B + 1:(b + 1) * B]) for b in range(3))
    p = sig(th[3 * B] + Wc @ th[3 * B + 1:])
    tiny = float(np.finfo(np.float32).tiny)
    l, q, col, ext = np.zeros(N), np.zeros((T, N)), np.zeros((T - 1, N)), np.zeros((T - 1, N))
    for i in range(N):
        paths = list(itertools.product((0, 1), repeat=T))
        lw = []
        for z in paths:
            lp = np.log(psi[i] if z[0] else 1.0 - psi[i])
            for t in range(1, T):
                pr1 = (1.0 - eps[i]) if z[t - 1] else gam[i]
                lp += np.log(pr1 if z[t] else 1.0 - pr1)
            for t, j in itertools.product(range(T), range(J)):
                if mask[i, t, j]:
                    pd = p[i, t, j] if z[t] else tiny
                    lp += np.log(pd) if Y32[i, t, j] != 0 else np.log1p(-pd)
            lw.append(lp)
        lw = np.array(lw)
        l[i] = lw.max() + np.log(np.exp(lw - lw.max()).sum())
        w, zz = np.exp(lw - l[i]), np.array(paths)
        q[:, i] = w @ zz
        col[:, i] = w @ ((zz[:, :-1] == 0) & (zz[:, 1:] == 1))
        ext[:, i] = w @ ((zz[:, :-1] == 1) & (zz[:, 1:] == 0))
    return l, q, col, ext


@pytest.mark.parametrize("T", [1, 2, 5])
def test_restatement_equals_brute_force_over_paths(T):
    rng = np.random.default_rng(T)
    X, W, Y = _data(rng, T=max(T, 3))   # a NaN visit, a whole season unobserved, a NaN obs covariate, a NaN site covariate
    W, Y = W[:, :T], Y[:, :T]
    for _ in range(3):
        th = rng.uniform(-2, 2, size=12)
        c = R.dyn_paths(X, W, Y, th)
        l, q, col, ext = _brute(X, W, Y, th)
        for name, got, want in (("l", c["l"], l), ("q", c["q"], q), ("col", c["col"], col), ("ext", c["ext"], ext)):
            assert got.shape == want.shape and np.max(np.abs(got - want), initial=0.0) < 1e-10, (name, np.max(np.abs(got - want)))
        assert np.array_equal(c["n_obs"], c["n_obs_period"].sum(0)) and c["n_obs"][4] == 0 and c["n_obs_period"][0, 2] == 0
        assert abs(c["l"][4]) < 1e-14 and np.allclose(c["q"][:, 4], R.propagated_prior(c["psi"], c["gamma"], c["eps"], T)[:, 4], atol=1e-14)


@pytest.mark.parametrize("T", [1, 4])
def test_site_terms_add_up_to_the_oracle_potential(T):
    rng = np.random.default_rng(10 + T)
    X, W, Y = _data(rng, N=40, T=max(T, 3), J=4)
    W, Y = W[:, :T], Y[:, :T]
    od = oracle.OracleData(X, W, Y, model="occu_dyn")
    for _ in range(3):
        th = rng.uniform(-2, 2, size=od.D)
        U, _ = od.potential_grad(th)
        want = -U - float(np.sum(stats.norm.logpdf(th)))
        assert abs(R.dyn_paths(X, W, Y, th)["l"].sum() - want) <= 1e-10 * max(1.0, abs(U))


@pytest.mark.parametrize("N", R.PARITY_N)
@pytest.mark.parametrize("ks,ko", R.PARITY_K)
@pytest.mark.parametrize("T", R.PARITY_T)
def test_float32_emulation_holds_half_the_gpu_bounds(T, ks, ko, N):
    """The kernel's recursions in np.float32 (positive-sum complements, pairs normalised from their parts) against the float64
    restatement at every (shape, theta) the GPU parity test uses: within HALF of its bounds."""
    X, W, Y, th = R.parity_case(T, ks, ko, N)
    worst = np.zeros(4)
    for b in range(th.shape[0]):
        c, e = R.dyn_paths(X, W, Y, th[b]), R.dyn_paths_f32(X, W, Y, th[b])
        bl, bp = R.bounds(c, R.RTOL)
        fr = [np.max(np.abs(e["l"] - c["l"]) / bl)] + [np.max(np.abs(e[k] - c[k]) / bp, initial=0.0) for k in ("q", "col", "ext")]
        worst = np.maximum(worst, fr)
    print(f"\n[f32 emulation T={T} K=({ks},{ko}) N={N}] max error / bound: log_lik {worst[0]:.3f}, z_prob {worst[1]:.3f}, "
          f"col_prob {worst[2]:.3f}, ext_prob {worst[3]:.3f}")
    assert np.all(worst <= 0.5), worst


def test_ffbs_draws_follow_the_smoothed_marginals_and_the_pairwise_terms():
    X, W, Y, centre = R.draws_case(2000, 4, 3, seed=5)
    c = R.dyn_paths(X, W, Y, centre)
    z = R.ffbs(c, np.random.default_rng(0), reps=20)
    q, col = np.broadcast_to(c["q"], z.shape), np.broadcast_to(c["col"], z[:, 1:].shape)
    s_q, n_q = R.standardised(z, q, 0.05, 0.95)
    s_c, n_c = R.standardised((z[:, :-1] == 0) & (z[:, 1:] == 1), col, 0.02, 0.98)
    # a sampler that ignores the dependence between seasons (independent Bernoulli(q) per cell) must fail the pairwise statistic
    zi = np.random.default_rng(1).uniform(size=z.shape) < q
    s_i, _ = R.standardised((zi[:, :-1] == 0) & (zi[:, 1:] == 1), col, 0.02, 0.98)
    print(f"\n[ffbs] cells in range {n_q} / {n_c}; standardised sums: z - q {s_q:.2f}, 1[col] - col {s_c:.2f}; independent draws {s_i:.1f}")
    assert n_q > 20000 and n_c > 10000
    assert abs(s_q) <= 4.5 and abs(s_c) <= 4.5
    assert abs(s_i) > 10


def test_finite_sample_turnover_by_hand():
    z = np.array([[0, 0, 1, 1], [1, 0, 1, 0], [1, 1, 1, 1]])[None, :, :, None]   # (1, T = 3, N = 4, 1)
    z = np.concatenate([z, np.ones_like(z)])                                      # a second draw with every site occupied throughout
    out = finite_sample_turnover({"z": z})
    assert set(out) == {"colonisation", "extinction"} and out["colonisation"].shape == out["extinction"].shape == (2, 2, 1)
    assert np.allclose(out["colonisation"][0, :, 0], [1 / 2, 2 / 2]) and np.allclose(out["extinction"][0, :, 0], [1 / 2, 0 / 2])
    assert np.all(np.isnan(out["colonisation"][1])) and np.all(out["extinction"][1] == 0)


@pytest.mark.parametrize("model", [occu, occu_rn, nmixture, occu_cop, occu_cs, occu_comb])
def test_refuses_every_model_but_occu_dyn(model):
    with pytest.raises(NotImplementedError, match=model.__biolith_amd_model__ + r"\b"):
        conditional_dynamics(model, None)


def test_refuses_a_non_model_and_points_here_from_conditional_occupancy():
    with pytest.raises(TypeError):
        conditional_dynamics(lambda **kw: None, None)
    with pytest.raises(TypeError):
        conditional_dynamics("occu_dyn", None)
    with pytest.raises(NotImplementedError, match="occu_dyn.*conditional_dynamics"):
        conditional_occupancy(occu_dyn, None)


def test_entry_point_is_declared_and_exported():
    assert "bl_path_posterior" in _ffi.EXPORTS
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "biolith_hip.h")).read()
    assert "int bl_path_posterior(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, float *log_lik, float *z_prob" in header


def test_end_to_end_inequalities_hold_for_the_reference_alone():
    """What test_gpu_dynamics.py asserts after fit -> conditional_dynamics, with the oracle's sampler and the float64 restatement in
    their place: the margins belong to the statistics, not to the device."""
    with contextlib.redirect_stdout(io.StringIO()):
        data, truth = simulate_dyn(**R.E2E)
    X, W, Y = data["site_covs"], data["obs_covs"], data["obs"]
    od = oracle.OracleData(X, W, Y, model="occu_dyn")
    draws = oracle.nuts_run(od, 300, 250, num_chains=2, seed=0)["draws"].reshape(-1, od.D)
    rng = np.random.default_rng(0)
    T, N = truth["z"].shape
    q, prior, z = np.zeros((T, N)), np.zeros((T, N)), []
    for th in draws:
        c = R.dyn_paths(X, W, Y, th)
        q += c["q"] / len(draws)
        prior += R.propagated_prior(c["psi"], c["gamma"], c["eps"], T) / len(draws)
        z.append(R.ffbs(c, rng)[0])
    b_q, b_prior = float(np.mean((q - truth["z"]) ** 2)), float(np.mean((prior - truth["z"]) ** 2))
    turn = finite_sample_turnover({"z": np.stack(z)[..., None]})
    col = float(np.nanmean(turn["colonisation"]))
    print(f"\n[dyn e2e, reference alone] Brier: z_prob {b_q:.4f}, propagated prior {b_prior:.4f}; mean z_prob {q.mean():.4f} "
          f"(true {truth['z'].mean():.4f}); colonisation {col:.4f} (true gamma {truth['gamma'].mean():.4f})")
    assert b_q < b_prior
    assert abs(q.mean() - truth["z"].mean()) < 0.1
    assert np.all(np.isfinite(turn["extinction"])) and abs(col - truth["gamma"].mean()) < 0.15
