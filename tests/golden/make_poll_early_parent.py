#!/usr/bin/env python3
"""Writes tests/golden/poll_early_parent.npz: the outputs of the launches of tests/test_gpu_poll_early.py as computed by the library
of the commit BEFORE the first poll round moved in front of the barrier (nuts_kernel.hpp: BL_POLL_EARLY, BL_POLL_REFILL) -- run on a
GPU box with that library:

    BIOLITH_HIP_LIB=/path/to/parent/libbiolith_hip.so python tests/golden/make_poll_early_parent.py [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                    # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the repository

import test_gpu_poll_early as t  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else t.PARENT
    ds = t.open_dataset()
    arrays = {}
    for (form, w, s) in t.SETS:
        r = t.run(ds, form, w, s)
        print(form, (w, s), r.kernel_name.rstrip(), "leapfrogs", np.asarray(r.n_leapfrog).sum(axis=0).tolist())
        for f in t.FIELDS:
            arrays[f"{form}/{w}_{s}/{f}"] = np.asarray(getattr(r, f))
    ds.close()
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
