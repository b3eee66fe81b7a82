"""Resources of bl_regional_totals' kernels, read from the built library's code objects as tests/test_kernel_resources.py reads them:
the main kernel keeps a site's staged covariates, its weight and the float64 recursion of the abundance draw in registers over all the
draws -- an array in scratch memory would be touched once per draw and covariate --, reduces across lanes without LDS (one region per
wave: nothing crosses waves before the finish kernel), and leaves room for at least 4 waves per SIMD."""
import re

from test_kernel_resources import kernel_metadata, needs_toolchain


@needs_toolchain
def test_regional_totals_kernels_stay_in_registers_without_lds(tmp_path_factory):
    meta = kernel_metadata(str(tmp_path_factory.getbasetemp()))
    mine = {n: v for n, v in meta.items() if re.match(r"_Z\d+bl_regional_totals_(?:finish_)?kernel", n)}
    assert sorted(re.search(r"bl_regional_totals_(?:finish_)?kernel", n).group(0) for n in mine) == \
        ["bl_regional_totals_finish_kernel", "bl_regional_totals_kernel"], sorted(mine)
    for name, (scratch, vgprs, static_lds) in mine.items():
        assert scratch == 0, (name, scratch)
        assert vgprs <= 128, (name, vgprs)   # at least 4 waves per SIMD
        assert static_lds == 0, (name, static_lds)
