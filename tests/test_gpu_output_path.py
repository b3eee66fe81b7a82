"""Workgroup 0's per-draw outputs and the staged launch constants (nuts_kernel.hpp: BL_OUT_DIRECT, BL_ABORT_DEFER).

Every lane of workgroup 0's control wave forms the address of ITS output once, in front of the loop -- lane d < D coordinate d of the
chain's draws, lanes D ... D + 3 num_steps, accept_prob, potential_energy and diverging -- and a sampling transition's end stores
through it; the adaptation windows' ends are staged once as well.  What can go wrong is an address: the chain's offset (chain x S), the
draw's index (first, last, a warm-up of zero in front), the stride of each array, the window that is read next.  So:

  * three chains in one launch against the same three chains launched one at a time by chain_offset (the same streams, chain 0 of a
    launch of one): every output equal bit for bit, for (num_warmup, num_samples) = (0, 1), (20, 2), (20, 33) and for a warm-up of 100,
    which closes four adaptation windows ([0, 14], [15, 39], [40, 89], [90, 99]: three staged ends are read in turn);
  * the same launches against the arrays the PARENT commit's library wrote for them (tests/golden/output_path_parent.npz, written by
    tests/golden/make_output_path_parent.py): the change moves stores, it must not move a bit;
  * in three forms of the sampler: the lean kernel on two workgroups per chain, the one-workgroup kernel (which keeps the parent's
    output code: profiles/NOTES.md -- it is held to the same arrays), the general kernel.

The cooperative stop is checked on the one-workgroup kernel and on two workgroups per chain with the bound of tests/test_gpu_nuts.py;
it holds for the synchronous read of the abort word (the default) and for the deferred sample (-DBL_ABORT_DEFER=1) alike."""
import os
import time

import numpy as np
import pytest

from biolith_amd.engine import OccuDataset
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

FIELDS = ("draws", "num_steps", "accept_prob", "diverging", "potential_energy", "step_size", "inv_mass", "n_leapfrog")
# form -> (workgroups per chain asked for, workgroups per chain expected, environment of the launch).  The one-workgroup KERNEL (no
# exchange) is what the host chooses by itself for a data set of this size; asked for by number, one workgroup runs the lean kernel
FORMS = {"lean_2wg": (2, 2, {}), "one_wg": (0, 1, {}), "general": (2, 2, {"BIOLITH_HIP_GENERAL": "1"})}
CASES = [(0, 1), (20, 2), (20, 33), (100, 3)]
CHAINS, SEED = 3, 11
PARENT = os.path.join(GOLDEN, "output_path_parent.npz")


def open_dataset():
    g = load_golden("small_3x3")
    return OccuDataset(g["site_covs"], g["obs_covs"], g["obs"])


def run(ds, form, warmup, samples, num_chains=CHAINS, chain_offset=0, setenv=os.environ.__setitem__, delenv=os.environ.pop):
    """One launch of `form`; the environment is put back before returning."""
    wgs, wgs_expected, env = FORMS[form]
    for var, value in env.items():
        setenv(var, value)
    try:
        r = ds.nuts(num_warmup=warmup, num_samples=samples, num_chains=num_chains, chain_offset=chain_offset, seed=SEED, wgs_per_chain=wgs)
    finally:
        for var in env:
            delenv(var, None)
    assert r.wgs_per_chain == wgs_expected, (form, r.wgs_per_chain)
    return r


@pytest.fixture(scope="module")
def ds():
    d = open_dataset()
    yield d
    d.close()


@pytest.fixture(scope="module")
def together(ds):
    """The three-chain launch of every form and case, computed once and shared by the two comparisons."""
    return {(form, w, s): run(ds, form, w, s) for form in FORMS for (w, s) in CASES}


@pytest.mark.parametrize("warmup,samples", CASES)
@pytest.mark.parametrize("form", list(FORMS))
def test_chains_of_one_launch_equal_chains_launched_alone(ds, together, form, warmup, samples):
    a = together[(form, warmup, samples)]
    assert a.draws.shape == (CHAINS, samples, ds.D) and np.isfinite(a.draws).all()
    for c in range(CHAINS):
        b = run(ds, form, warmup, samples, num_chains=1, chain_offset=c)
        for f in FIELDS:
            assert np.array_equal(getattr(a, f)[c], getattr(b, f)[0]), (form, warmup, samples, c, f)


@pytest.mark.parametrize("warmup,samples", CASES)
@pytest.mark.parametrize("form", list(FORMS))
def test_outputs_equal_the_parent_commits_bit_for_bit(together, form, warmup, samples):
    a = together[(form, warmup, samples)]
    z = np.load(PARENT)
    for f in FIELDS:
        want = z[f"{form}/{warmup}_{samples}/{f}"]
        got = np.asarray(getattr(a, f))
        assert got.dtype == want.dtype and got.shape == want.shape, (f, got.dtype, want.dtype, got.shape, want.shape)
        assert got.tobytes() == want.tobytes(), (form, warmup, samples, f)


def test_the_forms_are_the_kernels_they_are_named_for(together):
    lean, one, general = (together[(form, 20, 2)].kernel_name.rstrip() for form in ("lean_2wg", "one_wg", "general"))
    assert lean.endswith(", false, 5, true>"), lean            # one pair per lane, 5 visits, lean
    assert one.split(", ")[5] == "true", one                    # the lane-group / one-workgroup instantiation: no exchange
    assert general.endswith(", -1, false>"), general


@pytest.mark.parametrize("wgs", [0, 2])   # (0: the one-workgroup kernel, as above)
def test_abort_stops_a_running_kernel(ds, wgs):
    ds.launch(num_warmup=200000, num_samples=200000, num_chains=2, seed=0, wgs_per_chain=wgs)
    assert ds.wgs_per_chain() == (wgs or 1)
    assert not ds.done()
    t0 = time.time()
    ds.abort()
    with pytest.raises(Exception, match="aborted"):
        ds.wait()
    assert time.time() - t0 < 5.0
    # the handle stays usable
    r = ds.nuts(num_warmup=20, num_samples=10, num_chains=1, seed=0, wgs_per_chain=wgs)
    assert r.draws.shape == (1, 10, ds.D) and np.isfinite(r.draws).all()
