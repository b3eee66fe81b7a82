"""The control wave issues the first poll round of an exchange BEFORE the tick's first barrier and prepares the prior and the
speculative position in its shadow (nuts_kernel.hpp: BL_POLL_EARLY); a round that is not complete reloads only the loads whose tags
missed, each under its lanes' predicate (BL_POLL_REFILL).  Neither changes arithmetic, the order of a sum, the records' layout or the
protocol: a load issued early can only see a stale tag and be loaded again.  So every output must be what the PARENT commit's library
wrote, byte for byte (tests/golden/poll_early_parent.npz, written by tests/golden/make_poll_early_parent.py on that library):

  * the paired lean form (four 16-byte loads) at 2, 9 and 27 workgroups per chain and the general kernel (one batch of 8-byte loads,
    BIOLITH_HIP_GENERAL=1) at 9, `small_3x3`, 2 chains x (30 + 30);
  * the lean form at 9 with num_warmup = 0: the first tick of a launch is a tick without decisions in front of its early loads;
  * every launch above runs to its end, and the end is a tick whose decisions drop the evaluation in flight (`redo`): nothing is loaded
    on it, both barriers are still passed, and the leapfrog counters -- written behind the loop -- are the parent's.

The parent's arrays are the yardstick.  Beside them the lean kernel is held to the general kernel bit for bit at the shapes of
tests/test_gpu_poll_pairs.py (k = 2, 3, 8, 9, 16, 17, 27, 32 with 3 + 3 and 1 + 1 covariates: 8 -> 9 and 16 -> 17 change the number of
loads per round, 2 and 3 leave most lanes on clamped records), and k = 27 and 32 again with agent-scope stores
(BIOLITH_HIP_NO_LOCAL=1), which land later.  The product library has no retry counter; the stamps build's rounds per exchange at these
shapes are in profiles/NOTES.md and profiles/poll_early/rounds_test_shapes.txt: at k = 27 and 32 one exchange in five retries with
L2-local stores (80 and 119 refills per launch on chain 0's first workgroup), with agent-scope stores the lean kernel's first round
is longer and retries are RARE (2 per launch) while the general kernel retries 52 and 101 times -- so both store scopes are kept.

The default build ships BL_POLL_REFILL alone (BL_POLL_EARLY measured slower and is off: profiles/NOTES.md); this file passed on the
build with both switches on as well."""
import os

import numpy as np
import pytest

from biolith_amd.engine import OccuDataset
from conftest import GOLDEN, load_golden, quiet_simulate

pytestmark = pytest.mark.gpu

FIELDS = ("draws", "num_steps", "accept_prob", "potential_energy", "step_size", "inv_mass", "n_leapfrog", "diverging")
# form -> (workgroups per chain, environment of the launch)
FORMS = {"lean_2": (2, {}), "lean_9": (9, {}), "lean_27": (27, {}), "general_9": (9, {"BIOLITH_HIP_GENERAL": "1"})}
# (form, num_warmup, num_samples) of every set in the parent's file
SETS = [(form, 30, 30) for form in FORMS] + [("lean_9", 0, 8)]
CHAINS, SEED = 2, 7
PARENT = os.path.join(GOLDEN, "poll_early_parent.npz")

RUN = dict(num_warmup=30, num_samples=30, num_chains=2, seed=5)
WGS = [2, 3, 8, 9, 16, 17, 27, 32]
COVS = [(3, 3), (1, 1)]


def open_dataset():
    g = load_golden("small_3x3")
    return OccuDataset(g["site_covs"], g["obs_covs"], g["obs"])


def run(ds, form, warmup, samples, setenv=os.environ.__setitem__, delenv=os.environ.pop):
    """One launch of `form`; the environment is put back before returning."""
    wgs, env = FORMS[form]
    for var, value in env.items():
        setenv(var, value)
    try:
        r = ds.nuts(num_warmup=warmup, num_samples=samples, num_chains=CHAINS, seed=SEED, wgs_per_chain=wgs)
    finally:
        for var in env:
            delenv(var, None)
    assert r.wgs_per_chain == wgs, (form, r.wgs_per_chain)
    name = r.kernel_name.rstrip()
    assert name.endswith(", -1, false>" if env else ", false, 5, true>"), (form, name)
    return r


@pytest.fixture(scope="module")
def launches():
    """Every set of the parent's file, launched once on the library under test."""
    ds = open_dataset()
    try:
        return {(form, w, s): run(ds, form, w, s) for (form, w, s) in SETS}
    finally:
        ds.close()


@pytest.mark.parametrize("form,warmup,samples", SETS)
def test_outputs_equal_the_parent_commits_byte_for_byte(launches, form, warmup, samples):
    a = launches[(form, warmup, samples)]
    z = np.load(PARENT)
    for f in FIELDS:
        want = z[f"{form}/{warmup}_{samples}/{f}"]
        got = np.asarray(getattr(a, f))
        assert got.dtype == want.dtype and got.shape == want.shape, (f, got.dtype, want.dtype, got.shape, want.shape)
        assert got.tobytes() == want.tobytes(), (form, warmup, samples, f)


@pytest.mark.parametrize("form,warmup,samples", SETS)
def test_a_launch_runs_to_its_end_through_the_redo_tick(launches, form, warmup, samples):
    # the last transition's end drops the evaluation in flight and stops the run: every draw is there, and the counters written
    # behind the loop hold every leapfrog of the sampling phase
    a = launches[(form, warmup, samples)]
    assert a.draws.shape[:2] == (CHAINS, samples) and np.isfinite(a.draws).all()
    assert (a.num_steps >= 1).all()
    assert np.array_equal(np.asarray(a.n_leapfrog)[:, 1], a.num_steps.sum(axis=1))
    if warmup == 0:
        assert (np.asarray(a.n_leapfrog)[:, 0] == 0).all()


def _same(a, b):
    assert np.array_equal(a.draws, b.draws) and np.array_equal(a.num_steps, b.num_steps)
    assert np.array_equal(a.step_size, b.step_size) and np.array_equal(a.inv_mass, b.inv_mass)
    assert np.array_equal(a.accept_prob, b.accept_prob) and np.array_equal(a.diverging, b.diverging)
    assert np.array_equal(a.potential_energy, b.potential_energy) and np.array_equal(a.n_leapfrog, b.n_leapfrog)


def _lean_against_general(k, ks, ko, monkeypatch, **env):
    d = quiet_simulate(n_sites=k, n_site_covs=ks, n_obs_covs=ko, deployment_days_per_site=35, session_duration=7, random_seed=100 + k)[0]
    ds = OccuDataset(d["site_covs"], d["obs_covs"], d["obs"])
    try:
        for var, value in env.items():
            monkeypatch.setenv(var, value)
        monkeypatch.delenv("BIOLITH_HIP_GENERAL", raising=False)
        a = ds.nuts(wgs_per_chain=k, **RUN)
        assert ds.wgs_per_chain() == k and a.wgs_per_chain == k
        monkeypatch.setenv("BIOLITH_HIP_GENERAL", "1")
        b = ds.nuts(wgs_per_chain=k, **RUN)
        assert ds.wgs_per_chain() == k
        monkeypatch.delenv("BIOLITH_HIP_GENERAL", raising=False)
        na, nb = a.kernel_name.rstrip(), b.kernel_name.rstrip()
    finally:
        ds.close()
    assert na != nb and na.startswith(f"bl_nuts_kernel<{ks}, {ko}, true, 0, ") and na.endswith(", false, 5, true>"), (na, nb)
    assert nb.endswith(", -1, false>"), (na, nb)
    assert np.isfinite(a.draws).all()
    _same(a, b)
    return a


@pytest.mark.parametrize("ks,ko", COVS)
@pytest.mark.parametrize("k", WGS)
def test_lean_kernel_equals_the_general_kernel_bit_for_bit(k, ks, ko, monkeypatch):
    a = _lean_against_general(k, ks, ko, monkeypatch)
    assert a.chains_l2_local == 2


@pytest.mark.parametrize("ks,ko", COVS)
@pytest.mark.parametrize("k", [27, 32])
def test_agent_scope_stores(k, ks, ko, monkeypatch):
    a = _lean_against_general(k, ks, ko, monkeypatch, BIOLITH_HIP_NO_LOCAL="1")
    assert a.chains_l2_local == 0
