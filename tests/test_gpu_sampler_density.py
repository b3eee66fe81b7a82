"""The log density the persistent NUTS kernels compute inside their trees, at EVERY kept draw, against the float64 oracle.

bl_logp_grad (test_gpu_logp.py and its kin) shares only the per-site evaluation with the sampler: it picks its geometry for one chain
and adds the workgroups' partials on the host.  A launch picks workgroups per chain, sites per workgroup, the wide or the single-workgroup
form and lane groups for its own chain count, adds the partials in-kernel over the epoch-tagged exchange and runs per-form instantiations
(and bl_re_nuts_kernel for random effects).  Here every launch form runs ~150 + 150 transitions and the potential it stored for every
kept draw (float32 of the double U) must equal the oracle's U at the stored float32 draw to rtol (+ half a float32 ulp: tests/parity.py).
A slice summed at a stale theta, a dropped visit or a dropped site changes U by 5e-8 .. 2e-5 of itself at the headline
(tests/test_parity_bounds.py): the bounds of the plain model's family catch them; the statistical gates of test_gpu_nuts.py do not.

Every case asserts the form it was written for, so that the matrix cannot quietly collapse onto one kernel."""
import contextlib
import io

import numpy as np
import pytest

import oracle
from biolith_amd.distributions import LocScale
from biolith_amd.engine import OccuDataset
from conftest import CFG2, load_golden, quiet_simulate
from parity import assert_potential_parity, describe_launch, potential_at_draws, potential_ratio, relative_excess
from test_gpu_kernel_forms import CASES as FORM_CASES
from test_gpu_rn import _rn_data

pytestmark = pytest.mark.gpu

# rtol per model family: |U_kernel - U_oracle| <= rtol |U_oracle| + ulp32 / 2 at every kept draw.  Each is no looser than the family's
# bl_logp_grad bound; the measured maximum of (|dU| - ulp32 / 2) / |U| over the family's cases (MI355X) stands beside it.
RTOL = {
    "occu": 2e-7,      # bl_logp_grad bound 1e-6; measured 1.37e-7 (wgs_per_chain_1), 3.9e-8 at the headline
    "fp": 4e-7,        # bl_logp_grad bound 1e-6; measured 2.1e-7 (fp_constant: 52 visits a site, single workgroup)
    "dyn": 1e-7,       # bl_logp_grad bound 1e-6; measured 4.5e-8
    "species": 2e-7,   # bl_logp_grad bound 1e-6; measured 1.22e-7
    "rn": 1e-6,        # bl_logp_grad bound 1e-5; measured 4.2e-7 (rn_fp, through bl_re_nuts_kernel), 1.44e-7 on bl_nuts_kernel
    "cop": 3e-7,       # bl_logp_grad bound 2e-6; measured 1.28e-7
    "nmix": 2e-7,      # bl_logp_grad bound 2e-6; measured 9.4e-8
    "cs": 2e-7,        # bl_logp_grad bound 2e-6; measured 7.5e-8
    "re": 1e-7,        # bl_logp_grad bound 2e-6; measured 3.1e-8
    "rn_re": 3e-7,     # bl_logp_grad bound 1e-5; measured 1.32e-7
    "nmix_re": 2e-7,   # bl_logp_grad bound 2e-6; measured 9.5e-8
}
HEADLINE_KERNEL = "bl_nuts_kernel<3, 3, true, 0, 3, false, 5, true>"   # bench.py's occu workload (what rocprofv3 names)
W, S = 150, 150


def _sim(**kw):
    return quiet_simulate(**kw)[0]


def _data_kw(d, **kw):
    return d["site_covs"], d["obs_covs"], d["obs"], kw


def _missing():
    rng = np.random.default_rng(9)
    N, T, J = 1300, 2, 5
    X = rng.normal(size=(N, 3)); Wc = rng.normal(size=(N, T, J, 2)); Y = (rng.uniform(size=(1, N, T, J)) < 0.35) * 1.0
    X[::7, 1] = np.nan            # whole site masked
    Wc[::5, 1, 2, 0] = np.nan     # single visit masked
    Y[0, ::3, 0, :] = np.nan      # a period with no visits at all
    Y[0, 5] = np.nan              # a site with no data
    Y[0, 6] = 1.0                 # detections at every visit
    Y[0, 8] = 0.0                 # never detected
    Y[0, -1] = np.nan             # the last site without data (a half-filled last pair around it)
    return X.astype(np.float32), Wc.astype(np.float32), Y.astype(np.float32), {}


def _rn(n_sites, share, seed):
    X, Wc, Y = _rn_data(np.random.default_rng(seed), n_sites, 10, share)
    return X, Wc, Y, dict(model="occu_rn")


def _cop(fp):
    g = load_golden("cop_default")
    return _data_kw(g, model="occu_cop", fp_mode=fp, session_duration=g["session_duration"])


def _simulate(mod, fn, **kw):
    import importlib

    f = getattr(importlib.import_module(f"biolith_amd.models.{mod}"), fn)
    with contextlib.redirect_stdout(io.StringIO()):
        return f(**kw)[0]


def _form_case(name):
    d, kw = FORM_CASES[name]()
    return _data_kw(d, **kw)


def _per_form(f):
    """A per-form instantiation of bl_nuts_kernel, not the general kernel (", -1, false>")."""
    return f["kernel"].startswith("bl_nuts_kernel<") and not f["kernel"].rstrip().endswith(", -1, false>")


def _model(f):
    """The MODEL template argument of a bl_nuts_kernel instantiation (0 occu, 1 occu_rn, 2 false positives, 3 occu_cop, 4 nmixture)."""
    assert f["kernel"].startswith("bl_nuts_kernel<"), f
    return int(f["kernel"][len("bl_nuts_kernel<"):].split(",")[3])


# name -> (family, data builder -> (site_covs, obs_covs, obs, dataset kwargs), nuts kwargs, environment, check of the launch form)
MATRIX = {
    # ---- plain occu ----
    "headline_cfg2": ("occu", lambda: _data_kw(_sim(**CFG2)), dict(num_chains=4), {},
                      lambda f: f["kernel"] == HEADLINE_KERNEL and f["lds_staged"] and f["wgs_per_chain"] > 1),
    **{f"form_{n}": ("dyn" if n.startswith("dyn") else ("rn" if n == "rn" else "occu"), (lambda n=n: _form_case(n)), dict(num_chains=2), {},
                     _per_form) for n in sorted(FORM_CASES)},
    "dyn_8x4_general": ("dyn", lambda: _form_case("dyn_8x4"), dict(num_chains=2), {"BIOLITH_HIP_GENERAL": "1"},
                        lambda f: f["kernel"].rstrip().endswith(", 1, false>")),
    "grid_row_4_lane_groups": ("occu", lambda: _form_case("grid_row_4"), dict(num_chains=1), {},
                               lambda f: f["lane_group"][0] * f["lane_group"][1] > 1 and f["wgs_per_chain"] > 1),
    "wide_12800x90": ("occu", lambda: _data_kw(_sim(n_site_covs=2, n_obs_covs=1, n_sites=12800, deployment_days_per_site=7 * 90,
                                                    session_duration=7, random_seed=49)),
                      dict(num_chains=1, num_warmup=100, num_samples=60), {},
                      lambda f: f["wgs_per_chain"] > 32 and f["lds_staged"]),
    "unstaged_hbm_rows": ("occu", lambda: _data_kw(_sim(n_site_covs=2, n_obs_covs=1, n_sites=12800, deployment_days_per_site=7 * 90,
                                                        session_duration=7, random_seed=49)),
                          dict(num_chains=1, num_warmup=100, num_samples=60, wgs_per_chain=32), {},
                          lambda f: f["wgs_per_chain"] == 32 and not f["lds_staged"]),
    "single_workgroup": ("occu", lambda: _data_kw(load_golden("small_3x3")), dict(num_chains=2), {},
                         lambda f: f["wgs_per_chain"] == 1 and f["threads"] == 64 * 8 and f["lds_staged"]),
    **{f"wgs_per_chain_{k}": ("occu", lambda: _form_case("headline_like"), dict(num_chains=2, wgs_per_chain=k), {},
                              (lambda f, k=k: f["wgs_per_chain"] == k and f["threads"] != 64 * 8)) for k in (1, 2, 7)},
    "nine_chains_kmax16": ("occu", lambda: _data_kw(_sim(n_sites=3000, n_site_covs=2, n_obs_covs=2, deployment_days_per_site=42,
                                                         session_duration=7, random_seed=2)), dict(num_chains=9), {},
                           lambda f: 1 < f["wgs_per_chain"] <= 16),
    "missing_data": ("occu", _missing, dict(num_chains=2), {}, lambda f: f["wgs_per_chain"] >= 1),
    "laplace_priors": ("occu", lambda: _data_kw(load_golden("small_3x3"), prior_beta=LocScale(0.2, 0.7, "laplace"),
                                                prior_alpha=LocScale(-0.1, 1.5, "laplace")), dict(num_chains=2), {},
                       lambda f: f["wgs_per_chain"] >= 1),
    # ---- false positives ----
    "fp_constant": ("fp", lambda: _data_kw(load_golden("fp_constant"), model="occu_fp", fp_mode="constant"), dict(num_chains=2), {},
                    lambda f: _model(f) == 2),
    "fp_unoccupied": ("fp", lambda: _data_kw(load_golden("fp_unoccupied"), model="occu_fp", fp_mode="unoccupied"), dict(num_chains=2), {},
                      lambda f: _model(f) == 2),
    # ---- Royle-Nichols ----
    "rn_config4": ("rn", lambda: _data_kw(_simulate("occu_rn", "simulate_rn", n_sites=5000, n_site_covs=3, n_obs_covs=3,
                                                    deployment_days_per_site=70, session_duration=7, random_seed=0), model="occu_rn"),
                   dict(num_chains=2), {}, lambda f: f["wgs_per_chain"] == 32 and _model(f) == 1),
    "rn_split": ("rn", lambda: _rn(5000, 0.34, 11), dict(num_chains=2), {}, lambda f: f["wgs_per_chain"] == 32),
    "rn_sort_no_split": ("rn", lambda: _rn(10000, 0.05, 12), dict(num_chains=2), {}, lambda f: f["wgs_per_chain"] == 32),
    "rn_fp": ("rn", lambda: _data_kw(load_golden("rn_default"), model="occu_rn", re_fp_mode="constant", prior_fp=(2.0, 6.0)),
              dict(num_chains=2), {}, lambda f: f["wgs_per_chain"] >= 1),
    # ---- count models ----
    "cop": ("cop", lambda: _cop(None), dict(num_chains=2), {}, lambda f: _model(f) == 3),
    "cop_rate": ("cop", lambda: _cop("constant"), dict(num_chains=2), {}, lambda f: _model(f) == 3),
    "nmix_lds": ("nmix", lambda: _data_kw(load_golden("nmix_ref_test"), model="nmixture"), dict(num_chains=2), {},
                 lambda f: _model(f) == 4),
    "nmix_l2": ("nmix", lambda: _data_kw(load_golden("nmix_ref_test"), model="nmixture"), dict(num_chains=2), {"BIOLITH_HIP_NMIX_LDS": "0"},
                lambda f: _model(f) == 4),
    # ---- continuous scores, several species ----
    "cs": ("cs", lambda: _data_kw(load_golden("cs_default"), model="occu_cs"), dict(num_chains=2), {}, lambda f: f["wgs_per_chain"] >= 1),
    "three_species": ("species", lambda: _data_kw(_simulate("occu", "simulate", n_species=3, n_sites=250, n_site_covs=2, n_obs_covs=2,
                                                            deployment_days_per_site=42, random_seed=5)),
                      dict(num_chains=2), {}, lambda f: f["wgs_per_chain"] >= 1),
    # ---- random effects: bl_re_nuts_kernel ----
    "re_site_10000": ("re", lambda: _data_kw(_simulate("occu", "simulate", n_sites=10000, n_site_covs=3, n_obs_covs=3, deployment_days_per_site=70,
                                                       session_duration=7, site_random_effects=True, random_seed=0),
                                             model="occu_re", site_random_effects=True),
                      dict(num_chains=2), {}, lambda f: f["kernel"].startswith("bl_re_nuts_kernel") and f["wgs_per_chain"] >= 16),
    "re_site_obs_2000": ("re", lambda: _data_kw(_simulate("occu", "simulate", n_sites=2000, n_site_covs=3, n_obs_covs=3, deployment_days_per_site=70,
                                                          session_duration=7, site_random_effects=True, obs_random_effects=True, random_seed=0),
                                                model="occu_re", site_random_effects=True, obs_random_effects=True),
                         dict(num_chains=2), {}, lambda f: f["kernel"].startswith("bl_re_nuts_kernel")),
    "rn_re": ("rn_re", lambda: _data_kw(load_golden("rn_default"), model="occu_rn", max_abundance=100, site_random_effects=True,
                                        prior_site_re_sd=0.8), dict(num_chains=2), {},
              lambda f: f["kernel"].startswith("bl_re_nuts_kernel")),
    "nmix_re": ("nmix_re", lambda: (lambda g: _data_kw(g, model="nmixture", max_abundance=int(np.nanmax(g["obs"])) + 5, site_random_effects=True,
                                                       prior_site_re_sd=0.8))(load_golden("nmix_site_re")), dict(num_chains=2), {},
                lambda f: f["kernel"].startswith("bl_re_nuts_kernel")),
}


def _oracle_kw(kw):
    """The dataset's keyword arguments as the oracle takes them (a Laplace prior is a family there, not a LocScale)."""
    o = dict(kw)
    fam = [getattr(o.get(p), "family", "normal") for p in ("prior_beta", "prior_alpha")]
    if "laplace" in fam:
        for p in ("prior_beta", "prior_alpha"):
            v = o.get(p, (0.0, 1.0))
            o[p] = (float(v[0]), float(v[1]))
        o["prior_family"] = tuple(fam)
    return o


@pytest.mark.parametrize("case", sorted(MATRIX))
def test_sampler_potential_matches_the_oracle_at_every_draw(case, monkeypatch):
    family, build, nuts_kw, env, form_ok = MATRIX[case]
    X, Wc, Y, kw = build()
    for var in ("BIOLITH_HIP_GENERAL", "BIOLITH_HIP_NMIX_LDS"):
        monkeypatch.delenv(var, raising=False)
    for var, value in env.items():
        monkeypatch.setenv(var, value)
    ds = OccuDataset(X, Wc, Y, **kw)
    od = oracle.OracleData(X, Wc, Y, **_oracle_kw(kw))
    assert ds.D == od.D
    run = dict(num_warmup=W, num_samples=S, seed=3)
    run.update(nuts_kw)
    r = ds.nuts(**run)
    form = describe_launch(ds)
    assert form["kernel"] == r.kernel_name and form["wgs_per_chain"] == r.wgs_per_chain
    Uo = potential_at_draws(od, r)
    worst = float(np.max(potential_ratio(r.potential_energy, Uo, RTOL[family])))
    excess = relative_excess(r.potential_energy, Uo)
    print(f"\nPARITY {case} family={family} rtol={RTOL[family]:g} worst_ratio={worst:.3g} rel_excess={excess:.3g} "
          f"kernel={form['kernel']!r} k={form['wgs_per_chain']} threads={form['threads']} staged={form['lds_staged']} "
          f"l2_local={form['chains_on_l2_local_exchange']} lane_group={form['lane_group']} draws={Uo.size}")
    assert form_ok(form), (case, form)
    assert_potential_parity(r, Uo, RTOL[family], case)
    ds.close()
