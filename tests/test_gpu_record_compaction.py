"""The lean plain-model kernels of at most 8 coefficients and more than one workgroup per chain publish COMPACT exchange records
(nuts_kernel.hpp: BL_POLL_COMPACT): 8 granules of 8 bytes, {value, payload << 16 | epoch & 0xFFFF}.  The log-lik travels in the
payloads of granules 0 (bits 15:0) and 1 (bits 31:16), the abort word in granule 2's, the placement census (XCC id, its square, epoch
1 only) in granules 3 and 4.  Records are laid out as transposed pairs -- the 16-byte unit (sub, qp, d) holds granule d of the records
4 (2 qp) + sub and 4 (2 qp + 1) + sub -- and the control wave's lane (h, sub, d) polls the units (sub, 2 h + j, d), j = 0, 1, with two
16-byte loads per round.  Behind a complete round the lanes d = 1 reassemble the log-lik, four v_permlane32_swap hand lanes 0-31 the
values of q = 4 ... 7 and lanes 32-63 the log-lik of q = 0 ... 3, and every lane runs the f64 chain over q = 0 ... 7 that the 8-byte
form runs.  The general kernel (BIOLITH_HIP_GENERAL=1) keeps 16-granule records, one granule per load, and the same sums in the same
association: draws, trees, step sizes and metrics must be equal bit for bit (the method of tests/test_gpu_poll_pairs.py: k sites, one
per workgroup, so that every record carries a partial of its own).

Where the log-lik total comes out: in lane 33 (upper half, sub 0 after the folds, d = 1) for D = 8 (3 + 3 covariates), D = 4 (1 + 1)
and D = 2 (0 + 0) alike -- its chain runs in the lanes d = 1 of the upper half whatever D is, because its halves always travel in the
tags of granules 0 and 1.  (The paired form had it in lane 32 for D = 8 and in lanes 4 / 2 for D = 4 / 2.)  With D = 2 granule 1 is
both the last gradient component and the carrier of the log-lik's upper half.

Workgroups per chain: 2, 3 (only q = 0), 4, 5 (first record in the second half of a unit), 8, 9 (first second unit per lane: the second
load is issued from 9 on), 16, 17 (first record that arrives through the swap), 27 (the headline's: unwritten halves inside loads that
are issued), 28, 29 (first unit of the last load with both halves), 31, 32 (no unwritten half).

The general run of a (k, covariates) pair is made once and shared by the tests that compare against it."""
import time

import numpy as np
import pytest

from biolith_amd.engine import OccuDataset
from conftest import quiet_simulate

pytestmark = pytest.mark.gpu

RUN = dict(num_warmup=60, num_samples=40, num_chains=2, seed=5)
WGS = [2, 3, 4, 5, 8, 9, 16, 17, 27, 28, 29, 31, 32]
COVS = [(3, 3), (1, 1), (0, 0)]
FIELDS = ("draws", "num_steps", "step_size", "inv_mass", "accept_prob", "diverging")


def _same(a, b):
    for name in FIELDS:
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


@pytest.fixture(scope="module")
def shared():
    """(k, ks, ko) -> [handle, the general kernel's result for RUN]: one handle and one reference run per shape."""
    cache = {}
    yield cache
    for ds, _ in cache.values():
        ds.close()


def _handle_and_general(shared, k, ks, ko, monkeypatch, run=None):
    key = (k, ks, ko)
    if key not in shared:
        d = quiet_simulate(n_sites=k, n_site_covs=ks, n_obs_covs=ko, deployment_days_per_site=35, session_duration=7, random_seed=100 + k)[0]
        shared[key] = [OccuDataset(d["site_covs"], d["obs_covs"], d["obs"]), None]
    ds = shared[key][0]
    if run is not None or shared[key][1] is None:
        monkeypatch.setenv("BIOLITH_HIP_GENERAL", "1")
        b = ds.nuts(wgs_per_chain=k, **(run or RUN))
        monkeypatch.delenv("BIOLITH_HIP_GENERAL", raising=False)
        assert ds.wgs_per_chain() == k
        nb = b.kernel_name.rstrip()
        assert nb.endswith(", -1, false>"), nb
        assert b.record_bytes == 128, b.record_bytes   # (16 granules, one per load)
        if run is not None:
            return ds, b
        shared[key][1] = b
    return ds, shared[key][1]


def _lean(ds, k, ks, ko, monkeypatch, run=None, **env):
    for var, value in env.items():
        monkeypatch.setenv(var, value)
    monkeypatch.delenv("BIOLITH_HIP_GENERAL", raising=False)
    a = ds.nuts(wgs_per_chain=k, **(run or RUN))
    for var in env:
        monkeypatch.delenv(var, raising=False)
    assert ds.wgs_per_chain() == k and a.wgs_per_chain == k
    na = a.kernel_name.rstrip()
    # the lean one-pair-per-lane form of 5 visits at this capacity pair (a handle without covariates runs the kernels of capacity 1)
    assert na.startswith(f"bl_nuts_kernel<{max(ks, 1)}, {max(ko, 1)}, true, 0, ") and na.endswith(", false, 5, true>"), na
    assert a.record_bytes == 64, a.record_bytes
    assert np.isfinite(a.draws).all()
    return a


@pytest.mark.parametrize("ks,ko", COVS)
@pytest.mark.parametrize("k", WGS)
def test_compact_records_equal_the_general_kernel_bit_for_bit(k, ks, ko, shared, monkeypatch):
    ds, b = _handle_and_general(shared, k, ks, ko, monkeypatch)
    a = _lean(ds, k, ks, ko, monkeypatch)
    _same(a, b)
    # both chains' workgroups share an XCD and the census said so -- through the payload bits of granules 3 and 4
    assert a.chains_l2_local == 2


@pytest.mark.parametrize("ks,ko", COVS)
@pytest.mark.parametrize("k", [27, 32])
def test_agent_scope_stores(k, ks, ko, shared, monkeypatch):
    ds, b = _handle_and_general(shared, k, ks, ko, monkeypatch)
    a = _lean(ds, k, ks, ko, monkeypatch, BIOLITH_HIP_NO_LOCAL="1")
    _same(a, b)
    assert a.chains_l2_local == 0


@pytest.mark.parametrize("k", [2, 17])
def test_the_16_bit_tag_wraps(k, shared, monkeypatch):
    """More than 65 535 evaluations per chain, in warm-up and in sampling each: the tag epoch & 0xFFFF passes through 0 and repeats."""
    run = dict(num_warmup=16000, num_samples=16000, num_chains=2, seed=11)
    ds, b = _handle_and_general(shared, k, 3, 3, monkeypatch, run=run)
    a = _lean(ds, k, 3, 3, monkeypatch, run=run)
    print(f"k={k}: n_leapfrog per chain (warm-up, sampling) {a.n_leapfrog.tolist()}, kernel ms lean {a.kernel_ms:.1f} general {b.kernel_ms:.1f}")
    assert a.n_leapfrog.min() > 70000, a.n_leapfrog
    assert np.array_equal(a.n_leapfrog, b.n_leapfrog)
    _same(a, b)


def test_abort_through_the_payload_bit(shared, monkeypatch):
    """The host's stop request reaches every workgroup through granule 2's payload of member 0 (bound: tests/test_gpu_output_path.py)."""
    k = 27
    ds, _ = _handle_and_general(shared, k, 3, 3, monkeypatch)
    monkeypatch.delenv("BIOLITH_HIP_GENERAL", raising=False)
    ds.launch(num_warmup=200000, num_samples=200000, num_chains=2, seed=0, wgs_per_chain=k)
    assert ds.wgs_per_chain() == k
    assert not ds.done()
    t0 = time.time()
    ds.abort()
    with pytest.raises(Exception, match="aborted"):
        ds.wait()
    assert time.time() - t0 < 5.0
    assert ds.record_bytes() == 64   # (the kernel that was stopped says which records it published)
    # the handle stays usable
    r = _lean(ds, k, 3, 3, monkeypatch, run=dict(num_warmup=20, num_samples=10, num_chains=1, seed=0))
    assert r.draws.shape == (1, 10, ds.D)
