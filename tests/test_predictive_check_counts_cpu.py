"""predictive_check_counts without a GPU: the exports, the refusals and the argument checks -- all of them in front of any device call --
and the host path ``posterior_predictive_check_counts`` on hand-made site arrays against a brute-force float64 restatement of its
definition (``scipy.stats.poisson.pmf`` renormalised over 0..K, a Python loop over the groups).

Tolerance: E is a ratio of two sums of at most 128 non-negative float64 terms, each term good to a few ulp in both statements (the pmf
goes through exp and gammaln of arguments below ~60): rtol 1e-12 on E.  d_obs and d_rep follow from E by the same float64 expressions
summed in another order: rtol 1e-10."""
import numpy as np
import pytest
from scipy.stats import poisson

from biolith_amd import _ffi, models
from biolith_amd.evaluation import posterior_predictive_check_counts
from biolith_amd.evaluation.predictive_checks import _count_discrepancies, _expected_counts

PAIRS = [(g, s) for g in ("site", "revisit") for s in ("freeman-tukey", "chi-squared")]
MODELS = ["nmixture", "occu_rn", "occu_cop"]


class _NoPosterior:
    """Any use of the posterior -- the first step towards a device -- fails the test."""

    def get_samples(self):
        raise AssertionError("the posterior was read: the refusal came too late")


DATA = dict(site_covs=np.zeros((4, 1), np.float32), obs_covs=np.zeros((4, 1, 2, 1), np.float32), obs=np.zeros((1, 4, 1, 2), np.float32))


# ------------------------------------------------------------------------------------------ exports, refusals ----
def test_both_functions_and_the_entry_are_exported():
    from biolith_amd import evaluation, utils
    from biolith_amd.utils import predictive_check_counts

    assert "predictive_check_counts" in utils.__all__ and utils.predictive_check_counts is predictive_check_counts
    assert "posterior_predictive_check_counts" in evaluation.__all__ and callable(evaluation.posterior_predictive_check_counts)
    assert "bl_predictive_check_counts" in _ffi.EXPORTS
    assert "posterior_predictive_check_counts(m, predict(" in predictive_check_counts.__doc__


@pytest.mark.parametrize("name", ["occu", "occu_cs", "occu_comb", "occu_dyn"])
def test_other_models_are_refused_before_any_device_call(name):
    from biolith_amd.utils import predictive_check_counts

    with pytest.raises(NotImplementedError, match=rf"predictive_check_counts\(\): not built for {name} \(built: occu_rn, nmixture, occu_cop\)") as e:
        predictive_check_counts(getattr(models, name), _NoPosterior(), **DATA)
    assert ("use predictive_check" in str(e.value)) == (name == "occu")
    with pytest.raises(NotImplementedError, match=name):
        posterior_predictive_check_counts(getattr(models, name), {}, DATA["obs"], "site", "chi-squared")


def test_not_a_model_is_a_type_error():
    from biolith_amd.utils import predictive_check_counts

    with pytest.raises(TypeError, match="biolith_amd model"):
        predictive_check_counts(lambda **kw: None, _NoPosterior(), **DATA)


@pytest.mark.parametrize("bad", [dict(group_by="species"), dict(statistic="deviance")])
def test_bad_arguments_raise_the_host_checks_messages(bad):
    from biolith_amd.utils import predictive_check_counts

    with pytest.raises(ValueError) as host:
        posterior_predictive_check_counts(models.nmixture, {}, DATA["obs"], **bad)
    with pytest.raises(ValueError) as fused:
        predictive_check_counts(models.nmixture, _NoPosterior(), **DATA, **bad)
    assert str(fused.value) == str(host.value)


def test_missing_obs_and_a_wrong_shape_are_value_errors_before_any_device_call():
    from biolith_amd.utils import predictive_check_counts

    with pytest.raises(ValueError, match="obs is required"):
        predictive_check_counts(models.nmixture, _NoPosterior(), **{**DATA, "obs": None})
    with pytest.raises(ValueError, match="shape"):
        predictive_check_counts(models.occu_rn, _NoPosterior(), **{**DATA, "obs": np.zeros((1, 4, 1, 3), np.float32)})


# ------------------------------------------------------------------------------------------ the host path against brute force ----
n, S, N, T, J, K = 6, 2, 5, 2, 3, 7


def _sites(name, seed=0):
    """Hand-made predictive sites in predict()'s layout, observations with holes, and the function's extra arguments."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    obs = rng.poisson(2.0, (S, N, T, J)).astype(np.float64)
    ps, extra = {}, {}
    if name == "occu_cop":
        ps.update(psi=f32(rng.uniform(0.1, 0.9, (n, T, N, S))), rate_detection=f32(rng.uniform(0.2, 3.0, (n, J, T, N, S))),
                  y=rng.poisson(3.0, (n, J, T, N, S)).astype(np.int32))
        extra["session_duration"] = f32(rng.uniform(0.5, 9.0, (S, N, T, J)))
    else:
        ps.update(abundance=f32(rng.uniform(0.05, 9.0, (n, T, N, S))), prob_detection=f32(rng.uniform(0.05, 0.95, (n, J, T, N, S))))
        extra["max_abundance"] = K
        if name == "occu_rn":
            obs = np.minimum(obs, 1.0)
            ps["y"] = (rng.random((n, J, T, N, S)) < 0.4).astype(np.int32)
        else:
            ps["y"] = rng.binomial(5, 0.4, (n, J, T, N, S)).astype(np.int32)
    obs[rng.random(obs.shape) < 0.2] = np.nan
    obs[:, 1] = np.nan        # a site never seen
    obs[:, :, 1, 2] = np.nan  # a revisit never seen
    return ps, obs, extra


def _brute_expected(name, ps, extra, rates):
    """E (n, J, T, N, S) cell by cell: the definition as written, the restricted pmf from scipy."""
    E = np.zeros((n, J, T, N, S))
    for d in range(n):
        for j in range(J):
            for t in range(T):
                for i in range(N):
                    for s in range(S):
                        if name == "occu_cop":
                            psi, rate = float(ps["psi"][d, t, i, s]), float(ps["rate_detection"][d, j, t, i, s])
                            dur = extra["session_duration"]
                            dur = float(dur[s, i, t, j] if dur.ndim == 4 else dur[i, t, j])
                            f_c = float(rates["rate_fp_constant"][d]) if "rate_fp_constant" in rates else 0.0
                            f_u = float(rates["rate_fp_unoccupied"][d]) if "rate_fp_unoccupied" in rates else 0.0
                            E[d, j, t, i, s] = dur * (psi * rate + (1.0 - psi) * f_u + f_c)
                            continue
                        lam, p = float(ps["abundance"][d, t, i, s]), float(ps["prob_detection"][d, j, t, i, s])
                        support = np.arange(K + 1)
                        pi = poisson.pmf(support, lam)
                        pi = pi / pi.sum()
                        if name == "nmixture":
                            E[d, j, t, i, s] = (pi * support).sum() * p
                        else:
                            f = float(rates["prob_fp_constant"][d]) if "prob_fp_constant" in rates else 0.0
                            E[d, j, t, i, s] = 1.0 - (1.0 - f) * (pi * (1.0 - p) ** support).sum()
    return E


def _brute_discrepancies(E, y, obs, group_by, statistic):
    stat = {"freeman-tukey": lambda o, e: (np.sqrt(o) - np.sqrt(e)) ** 2, "chi-squared": lambda o, e: (o - e) ** 2 / (e + 1e-10)}[statistic]
    d_obs, d_rep = np.zeros(n), np.zeros(n)
    groups = [(s, i) for s in range(S) for i in range(N)] if group_by == "site" else [(s, t, j) for s in range(S) for t in range(T) for j in range(J)]
    for d in range(n):
        for g in groups:
            o = r = e = 0.0
            cells = [(g[0], g[1], t, j) for t in range(T) for j in range(J)] if group_by == "site" else [(g[0], i, g[1], g[2]) for i in range(N)]
            for s, i, t, j in cells:
                if not np.isnan(obs[s, i, t, j]):
                    o += obs[s, i, t, j]; r += float(y[d, j, t, i, s]); e += E[d, j, t, i, s]
            d_obs[d] += stat(o, e)
            d_rep[d] += stat(r, e)
    return d_obs, d_rep


CASES = [("nmixture", {}), ("occu_rn", {}), ("occu_rn", {"prob_fp_constant": 0.1}), ("occu_cop", {}),
         ("occu_cop", {"rate_fp_constant": 0.3}), ("occu_cop", {"rate_fp_unoccupied": 0.3})]


@pytest.mark.parametrize("name,fp", CASES, ids=[c[0] + "".join("-" + k for k in c[1]) for c in CASES])
def test_the_host_path_equals_the_brute_force_restatement(name, fp):
    ps, obs, extra = _sites(name)
    rates = {k: np.float32(v) * np.linspace(0.5, 1.5, n).astype(np.float32) for k, v in fp.items()}
    model = getattr(models, name)
    want_E = _brute_expected(name, ps, extra, rates)
    got_E = _expected_counts(name, {**ps, **rates}, extra.get("session_duration"), extra.get("max_abundance", 100), obs.shape)
    err = np.max(np.abs(got_E - want_E) / np.abs(want_E))
    print(f"{name} {sorted(fp)} E: max rel err {err:.3e}")
    np.testing.assert_allclose(got_E, want_E, rtol=1e-12, atol=0)
    for g, s in PAIRS:
        d_obs, d_rep = _brute_discrepancies(want_E, ps["y"], obs, g, s)
        got = _count_discrepancies(model, ps, obs, g, s, extra.get("session_duration"), extra.get("max_abundance", 100), rates)
        np.testing.assert_allclose(got[0], d_obs, rtol=1e-10, atol=0, err_msg=f"d_obs {g} {s}")
        np.testing.assert_allclose(got[1], d_rep, rtol=1e-10, atol=0, err_msg=f"d_rep {g} {s}")
        # the rate as a keyword and the rate merged into the samples are the same call
        p_kw = posterior_predictive_check_counts(model, ps, obs, g, s, **extra, **rates)
        p_in = posterior_predictive_check_counts(model, {**ps, **rates}, obs, g, s, **extra)
        assert p_kw == p_in == float(np.mean(got[1] > got[0])) and 0.0 <= p_kw <= 1.0


def test_session_duration_with_and_without_the_species_axis():
    ps, obs, extra = _sites("occu_cop")
    shared = extra["session_duration"][0]                                    # (N, T, J)
    both = np.broadcast_to(shared, (S, N, T, J))
    for g, s in PAIRS:
        a = _count_discrepancies(models.occu_cop, ps, obs, g, s, shared, 100, {})
        b = _count_discrepancies(models.occu_cop, ps, obs, g, s, both, 100, {})
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    ones = _count_discrepancies(models.occu_cop, ps, obs, "site", "chi-squared", None, 100, {})
    assert np.array_equal(ones[0], _count_discrepancies(models.occu_cop, ps, obs, "site", "chi-squared", np.ones((N, T, J)), 100, {})[0])


@pytest.mark.parametrize("name", ["nmixture", "occu_rn"])
@pytest.mark.parametrize("lam,cap", [(3.0e4, 100), (1e-6, 100), (float(np.finfo(np.float32).max), 127), (0.0, 5)])
def test_the_truncated_sums_stay_finite(name, lam, cap):
    # lambda^n / n! overflows float64 at lambda = 3e4, n = 100; exp(-lambda) underflows from lambda = 745 on
    ps, obs, _ = _sites(name)
    ps["abundance"] = np.full_like(ps["abundance"], lam)
    E = _expected_counts(name, ps, None, cap, obs.shape)
    assert np.isfinite(E).all() and (E >= 0).all()
    if name == "nmixture":   # the restricted mean tends to K above it and to lambda below it
        m = E / ps["prob_detection"].astype(np.float64)
        np.testing.assert_allclose(m, min(lam, cap) if lam < 1 or lam > 1e3 else m, rtol=5e-3)
    for g, s in PAIRS:
        p = posterior_predictive_check_counts(getattr(models, name), ps, obs, g, s, max_abundance=cap)
        d = _count_discrepancies(getattr(models, name), ps, obs, g, s, None, cap, {})
        assert np.isfinite(d[0]).all() and np.isfinite(d[1]).all() and 0.0 <= p <= 1.0
