"""The sampler's potential-parity bound has teeth (oracle only, no GPU).

At the headline data (config 2: 10 000 sites x 5 visits) and points of the typical set, potentials with a fault of the kind an in-kernel
evaluation could make -- one never-detected site dropped, one visit dropped, one workgroup's 313-site slice summed at the theta of one
leapfrog away (a stale exchange) -- must be rejected by the plain model's rtol of tests/test_gpu_sampler_density.py; the exact potential
rounded through float32 at a float32 theta (what the kernel stores) must be accepted."""
import json
import os
import re

import numpy as np
import pytest

import oracle
from conftest import CFG2, GOLDEN, quiet_simulate
from parity import potential_ratio

RTOL_OCCU = 2e-7    # = test_gpu_sampler_density.RTOL["occu"] (that module is GPU-marked; the value is checked against it below)
SLICE = 313         # sites per workgroup at the headline: ceil(10 000 / 32)


@pytest.fixture(scope="module")
def cfg2():
    data, _, _ = quiet_simulate(**CFG2)
    fx = json.load(open(os.path.join(GOLDEN, "oracle_posterior_cfg2.json")))
    rng = np.random.default_rng(3)
    th = np.array(fx["mean"]) + np.array(fx["sd"]) * rng.normal(size=(4, 8))   # typical-set points
    return data, fx, th.astype(np.float32).astype(np.float64), rng


def _od(data, obs=None, sites=slice(None)):
    return oracle.OracleData(data["site_covs"][sites], data["obs_covs"][sites], (data["obs"] if obs is None else obs)[:, sites])


def _U(od, th):
    return od.potential_grad(th)[0]


def test_rtol_is_the_samplers():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_sampler_density.py")).read()
    m = re.search(r'"occu": ([0-9.e+-]+),', src)
    assert m and float(m.group(1)) == RTOL_OCCU


def test_float32_store_is_accepted(cfg2):
    data, _, th, _ = cfg2
    U = _U(_od(data), th)
    stored = U.astype(np.float32).astype(np.float64)
    assert np.all(potential_ratio(stored, U, RTOL_OCCU) <= 1.0)
    # ... and so is the exact value, and a rounding error of the size bl_logp_grad shows (~1e-8)
    assert np.all(potential_ratio(U * (1 + 1e-8), U, RTOL_OCCU) <= 1.0)


def test_dropped_never_detected_site_is_rejected(cfg2):
    data, _, th, _ = cfg2
    U = _U(_od(data), th)
    obs = np.array(data["obs"])
    never = np.nonzero(np.nansum(obs[0], axis=(1, 2)) == 0)[0]
    obs[0, never[len(never) // 2]] = np.nan
    Uf = _U(_od(data, obs), th).astype(np.float32).astype(np.float64)
    r = potential_ratio(Uf, U, RTOL_OCCU)
    assert np.all(r > 1.0), r


def test_dropped_visit_is_rejected(cfg2):
    data, _, th, _ = cfg2
    U = _U(_od(data), th)
    obs = np.array(data["obs"])
    det = np.argwhere(obs[0] == 1.0)
    n, t, j = det[len(det) // 2]
    obs[0, n, t, j] = np.nan
    Uf = _U(_od(data, obs), th).astype(np.float32).astype(np.float64)
    r = potential_ratio(Uf, U, RTOL_OCCU)
    assert np.all(r > 1.0), r


def test_stale_slice_is_rejected(cfg2):
    """One 313-site slice summed at the theta of one leapfrog away: theta' = theta + eps M^-1 p, p ~ N(0, M), with the step size and
    inverse mass the oracle's sampler adapted at this posterior (oracle_posterior_cfg2.json).  The slice enters U only through its
    likelihood; the prior is the full theta's."""
    data, fx, th, rng = cfg2
    U = _U(_od(data), th)
    eps, minv = float(np.mean(fx["step_size"])), np.mean(np.array(fx["inv_mass"]), axis=0)
    th2 = (th + eps * np.sqrt(minv) * rng.normal(size=th.shape)).astype(np.float32).astype(np.float64)
    w = 16
    sl = slice(w * SLICE, (w + 1) * SLICE)
    empty = np.full_like(np.asarray(data["obs"]), np.nan)
    prior = _od(data, empty, sl)   # the same sites without observations: the prior alone
    like_now = _U(_od(data, sites=sl), th) - _U(prior, th)
    like_stale = _U(_od(data, sites=sl), th2) - _U(prior, th2)
    Uf = (U - like_now + like_stale).astype(np.float32).astype(np.float64)
    r = potential_ratio(Uf, U, RTOL_OCCU)
    print("stale slice: |dU| / |U| =", np.abs(Uf - U) / np.abs(U), "ratio to the bound", r)
    assert np.all(r > 1.0), r
