"""Resources of bl_response_curves' kernels, read from the built library's code objects as tests/test_kernel_resources.py reads them:
the site kernel keeps a site's staged covariates and its weight in registers over all the draws and values, the obs kernel a visit's
covariates and its block of float64 accumulators -- the covariate that is replaced is selected by comparing the unrolled loops' own
index with it, never by indexing the array with it, which would put the array in scratch memory --; both reduce across lanes without
LDS (one run of 64 sites per wave: nothing crosses waves before the finish kernel) and leave room for at least 4 waves per SIMD."""
import re

from test_kernel_resources import kernel_metadata, needs_toolchain

KERNELS = ["bl_response_curves_finish_kernel", "bl_response_curves_obs_kernel", "bl_response_curves_site_kernel"]


@needs_toolchain
def test_response_curves_kernels_stay_in_registers_without_lds(tmp_path_factory):
    meta = kernel_metadata(str(tmp_path_factory.getbasetemp()))
    mine = {n: v for n, v in meta.items() if re.match(r"_Z\d+bl_response_curves_(?:site|obs|finish)_kernel", n)}
    assert sorted(re.search(r"bl_response_curves_(?:site|obs|finish)_kernel", n).group(0) for n in mine) == KERNELS, sorted(mine)
    for name, (scratch, vgprs, static_lds) in mine.items():
        print(name, "scratch", scratch, "vgprs", vgprs, "static LDS", static_lds)
        assert scratch == 0, (name, scratch)
        assert vgprs <= 128, (name, vgprs)   # at least 4 waves per SIMD
        assert static_lds == 0, (name, static_lds)
