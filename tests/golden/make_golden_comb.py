#!/usr/bin/env python3
"""Generate tests/golden/simulate_comb_index.json by IMPORTING the reference's simulate_comb (build container only).

As make_golden.py: jax / numpyro / funsor are served as stubs at import time (the reference's simulators are pure NumPy), and
only DATA is written -- each case's keyword arguments, its printed lines, the SHA-256 of every returned array and the
scalars of true_params.

Run:  python tests/golden/make_golden_comb.py        (needs the reference; not run on the GPU box)
"""
import contextlib
import io
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import HERE, load_reference_simulate, sha  # noqa: E402

CASES = {
    "comb_default": {},
    "comb_missing": dict(simulate_missing=True),
    "comb_missing_3periods": dict(simulate_missing=True, n_periods=3),
    "comb_two_species": dict(simulate_missing=True, n_species=2, n_sites=30),
    "comb_effects": dict(site_random_effects=True, PC_obs_random_effects=True, ARU_obs_random_effects=True),
    "comb_fp_rates": dict(ARU_prob_fp_constant=0.05, ARU_prob_fp_unoccupied=0.1, random_seed=3),
    "comb_shapes": dict(n_site_covs=3, n_PC_covs=0, n_ARU_covs=2, n_sites=20, PC_replicates=2, ARU_replicates=5,
                        scores_replicates=4, random_seed=7, simulate_missing=True),
}


def record(value):
    if isinstance(value, np.ndarray):
        return dict(sha=sha(value), shape=list(value.shape), dtype=str(value.dtype))
    return value


def main():
    load_reference_simulate()
    simulate_comb = sys.modules["biolith.models.occu_comb"].simulate_comb
    index = {}
    for name, kw in CASES.items():
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            data, truth = simulate_comb(**kw)
        index[name] = dict(kwargs=kw, stdout=buf.getvalue(), data={k: record(v) for k, v in data.items()},
                           truth={k: record(v) for k, v in truth.items()})
    with open(os.path.join(HERE, "simulate_comb_index.json"), "w") as f:
        json.dump(index, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
