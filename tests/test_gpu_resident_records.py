"""The lean plain-model sampler kernels keep a lane's site-pair record in registers for the whole launch (nuts_kernel.hpp:
BL_RESIDENT_REC; occu_device.hpp: bl_load_resident_rec / bl_eval_sites_rec) instead of reading it from LDS at every evaluation.  The
general kernel (BIOLITH_HIP_GENERAL=1) still reads LDS every tick and runs the same arithmetic in the same order, so draws, trees,
divergences, step sizes and metrics must be equal bit for bit -- for every compile-time J form, at both ends of the record sizes, with
an odd slice (dummy second site), with lanes and whole waves that have no pair, with a workgroup that has no site, at both compute-wave
counts, and with masked visits (the masks live in the record).

What these tests can and cannot see: both kernels evaluate a pair with the same bl_pair_* pieces (occu_device.hpp), so a difference
here is a fault of the one-time load -- the record's index and its clamp, the dummy-site mask, the pair-valid predicate -- or of keeping
the record across ticks.  A slip in the shared arithmetic itself would move both sides alike; that is held by the parity tests against
the float64 oracle (tests/test_gpu_logp.py, tests/test_gpu_nuts.py) and by smoke().

Every launch names its workgroups per chain: a chain of one workgroup would take the lane-group kernel, which has no resident record."""
import numpy as np
import pytest

from biolith_amd.engine import OccuDataset
from conftest import quiet_simulate

pytestmark = pytest.mark.gpu

RUN = dict(num_warmup=60, num_samples=40, num_chains=2, seed=5)   # crosses adaptation-window ends and many transition ends


def _data(n_sites, J, ks=3, ko=3, seed=7):
    return quiet_simulate(n_sites=n_sites, n_site_covs=ks, n_obs_covs=ko, deployment_days_per_site=7 * J, session_duration=7, random_seed=seed)[0]


def _lean_against_general(d, J, monkeypatch, wgs, cwaves=None, **more):
    ds = OccuDataset(d["site_covs"], d["obs_covs"], d["obs"])
    try:
        monkeypatch.delenv("BIOLITH_HIP_GENERAL", raising=False)
        if cwaves is not None:
            monkeypatch.setenv("BIOLITH_HIP_CWAVES", str(cwaves))
        a = ds.nuts(wgs_per_chain=wgs, **RUN, **more)
        assert ds.wgs_per_chain() == wgs
        monkeypatch.setenv("BIOLITH_HIP_GENERAL", "1")
        b = ds.nuts(wgs_per_chain=wgs, **RUN, **more)
        monkeypatch.delenv("BIOLITH_HIP_GENERAL", raising=False)
        na, nb = a.kernel_name.rstrip(), b.kernel_name.rstrip()
    finally:
        ds.close()
    # the lean one-pair-per-lane form of exactly this J (the resident family), then the general kernel
    assert na != nb and na.endswith(f", false, {J}, true>") and nb.endswith(", -1, false>"), (na, nb)
    if cwaves is not None:
        assert f", true, 0, {cwaves}, false, " in na, na
    assert np.array_equal(a.draws, b.draws) and np.array_equal(a.num_steps, b.num_steps)
    assert np.array_equal(a.diverging, b.diverging)
    assert np.array_equal(a.step_size, b.step_size) and np.array_equal(a.inv_mass, b.inv_mass)
    assert np.isfinite(a.draws).all()


@pytest.mark.parametrize("J", [1, 2, 3, 4, 5, 6, 8])
def test_every_visit_count_form(J, monkeypatch):
    # 700 sites on 2 workgroups: 175 pairs each -- two full waves and 47 lanes of the third
    _lean_against_general(_data(700, J), J, monkeypatch, wgs=2)


@pytest.mark.parametrize("ks,ko", [(1, 1), (4, 4)])
def test_smallest_and_largest_record(ks, ko, monkeypatch):
    _lean_against_general(_data(700, 5, ks, ko, seed=9), 5, monkeypatch, wgs=2)


def test_largest_record_of_all(monkeypatch):
    # 4 + 4 covariates at 8 visits: 96 floats per lane, the bound of what is kept resident
    _lean_against_general(_data(700, 8, 4, 4, seed=10), 8, monkeypatch, wgs=2)


def test_odd_slice_has_a_dummy_second_site(monkeypatch):
    # 701 sites on 2 workgroups: slices of 351 (its last pair holds one site and the zero-filled dummy) and 350
    _lean_against_general(_data(701, 5, seed=3), 5, monkeypatch, wgs=2)


def test_lanes_and_a_whole_wave_without_a_pair(monkeypatch):
    # 700 sites on 3 workgroups: 117 / 117 / 116 pairs -- the second wave is part empty, the third has no pair at all
    _lean_against_general(_data(700, 5, seed=4), 5, monkeypatch, wgs=3)


def test_a_workgroup_without_sites(monkeypatch):
    # 25 sites on 6 workgroups: five slices of 5 sites (odd), the sixth empty -- its lanes' one-time load stays inside the staged region
    _lean_against_general(_data(25, 5, seed=6), 5, monkeypatch, wgs=6)


def test_four_compute_waves(monkeypatch):
    # 900 sites on 2 workgroups of FOUR compute waves: 225 pairs per workgroup, more than three waves hold
    _lean_against_general(_data(900, 5, seed=8), 5, monkeypatch, wgs=2, cwaves=4)


def test_masked_visit_and_fully_masked_site(monkeypatch):
    d = _data(700, 5, seed=12)
    obs = np.array(d["obs"], dtype=np.float64)
    rows = obs.reshape(-1, 5)   # one species, one period: a row per site
    assert rows.shape[0] == 700
    rows[3, 1] = np.nan         # one visit
    rows[10, :] = np.nan        # a site nobody visited
    rows[699, :] = np.nan       # ... and the last site of the last slice
    d = dict(d, obs=obs)
    _lean_against_general(d, 5, monkeypatch, wgs=2)

