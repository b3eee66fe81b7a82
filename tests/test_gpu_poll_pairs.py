"""The lean sampler kernels of at most 8 coefficients lay a workgroup's exchange record out in 16-byte pairs and poll it with four
16-byte loads per round (nuts_kernel.hpp: BL_POLL_PAIRS): granule v of a record sits at position v < 8 ? 2 v : 2 (v - 8) + 1, the
control wave's lane (h, sub, c2) reads pair c2 of record 4 (2 q' + h) + sub, and one v_permlane32_swap per load puts the values back
into the lanes and the order in which the 8-byte form summed them.  The general kernel (BIOLITH_HIP_GENERAL=1) keeps the 8-byte form
-- one granule per load, records in their plain order -- and the same f64 sums in the same association, so draws, trees, step sizes and
metrics must be equal bit for bit, compared the way tests/test_gpu_kernel_forms.py does.

Workgroups per chain: 2, 3 (one load, only the lower half real), 8, 9 (one load / two loads, both halves), 16, 17, 27 (the headline's),
32 (every load, no clamp) -- one and several loads, odd and even counts of record groups, records clamped to the last one in a load that
is issued and loads that are skipped.  Covariates: 3 + 3 (8 coefficients: log-lik, abort flag and census words come out of lanes
32 ... 35) and 1 + 1 (4 coefficients: out of lanes 4 ... 7).

Sites: the host launches the lean one-pair-per-lane form for ANY site count once the workgroups per chain are named (choose_geometry
takes neither the one-workgroup kernel nor lane groups then: 5 visits), so the smallest dataset is set by what the exchange is to
show: k sites, one per workgroup -- every one of the k records then carries a partial of its own; with fewer the surplus records are
zeros, which a wrong record index would not disturb."""
import numpy as np
import pytest

from biolith_amd.engine import OccuDataset
from conftest import quiet_simulate

pytestmark = pytest.mark.gpu

RUN = dict(num_warmup=60, num_samples=40, num_chains=2, seed=5)
WGS = [2, 3, 8, 9, 16, 17, 27, 32]
COVS = [(3, 3), (1, 1)]


def _same(a, b):
    assert np.array_equal(a.draws, b.draws) and np.array_equal(a.num_steps, b.num_steps)
    assert np.array_equal(a.step_size, b.step_size) and np.array_equal(a.inv_mass, b.inv_mass)
    assert np.array_equal(a.accept_prob, b.accept_prob) and np.array_equal(a.diverging, b.diverging)


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
    # the lean one-pair-per-lane form of 5 visits at this capacity pair (paired records), then the general kernel (8-byte form)
    assert na != nb and na.startswith(f"bl_nuts_kernel<{ks}, {ko}, true, 0, ") and na.endswith(", false, 5, true>"), (na, nb)
    assert nb.endswith(", -1, false>"), (na, nb)
    assert np.isfinite(a.draws).all()
    _same(a, b)
    return a


@pytest.mark.parametrize("ks,ko", COVS)
@pytest.mark.parametrize("k", WGS)
def test_paired_records_equal_the_general_kernel_bit_for_bit(k, ks, ko, monkeypatch):
    a = _lean_against_general(k, ks, ko, monkeypatch)
    assert a.chains_l2_local == 2   # (both chains' workgroups share an XCD: workgroup-scope stores, the L2-local exchange)


@pytest.mark.parametrize("ks,ko", COVS)
@pytest.mark.parametrize("k", [27, 32])
def test_agent_scope_stores(k, ks, ko, monkeypatch):
    a = _lean_against_general(k, ks, ko, monkeypatch, BIOLITH_HIP_NO_LOCAL="1")
    assert a.chains_l2_local == 0


def test_an_odd_pitch_is_rounded_up_to_keep_pairs_aligned(monkeypatch):
    # 17 granules between records would put every second record's pairs 8 bytes off a 16-byte boundary: the host makes it 18
    _lean_against_general(9, 3, 3, monkeypatch, BIOLITH_HIP_PITCH="17")
