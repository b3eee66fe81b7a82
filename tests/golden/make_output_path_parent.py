#!/usr/bin/env python3
"""Writes tests/golden/output_path_parent.npz: the outputs of the small launches of tests/test_gpu_output_path.py as computed by the
library of the commit BEFORE the per-draw stores moved (nuts_kernel.hpp: BL_OUT_DIRECT) -- run on a GPU box with that library:

    BIOLITH_HIP_LIB=/path/to/parent/libbiolith_hip.so python tests/golden/make_output_path_parent.py [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                    # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the repository

import test_gpu_output_path as t  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else t.PARENT
    ds = t.open_dataset()
    arrays = {}
    for form in t.FORMS:
        for (w, s) in t.CASES:
            r = t.run(ds, form, w, s)
            print(form, (w, s), r.kernel_name.rstrip(), "leapfrogs", r.n_leapfrog.sum(axis=0).tolist())
            for f in t.FIELDS:
                arrays[f"{form}/{w}_{s}/{f}"] = np.asarray(getattr(r, f))
    ds.close()
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
