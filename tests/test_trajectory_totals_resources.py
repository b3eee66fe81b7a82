"""Resources of bl_trajectory_totals' kernels, read from the built library's code objects as tests/test_kernel_resources.py reads them:
the main kernel keeps a site's covariates (float64, the capacity of an occu_dyn handle), its weight, the six rates and the pair
(pi, q) in registers over all the draws and periods -- T is a run-time value and nothing is kept per period --, the finish kernel
holds the 32 partials it loads ahead of its additions and selects a row's output by a chain of compares over the unrolled outputs,
never by indexing the parameter block with the row; both reduce without LDS and leave room for at least 4 waves per SIMD."""
import re

from test_kernel_resources import kernel_metadata, needs_toolchain

KERNELS = ["bl_trajectory_totals_finish_kernel", "bl_trajectory_totals_kernel"]


@needs_toolchain
def test_trajectory_totals_kernels_stay_in_registers_without_lds(tmp_path_factory):
    meta = kernel_metadata(str(tmp_path_factory.getbasetemp()))
    mine = {n: v for n, v in meta.items() if re.match(r"_Z\d+bl_trajectory_totals_(?:finish_)?kernel", n)}
    assert sorted(re.search(r"bl_trajectory_totals_(?:finish_)?kernel", n).group(0) for n in mine) == KERNELS, sorted(mine)
    for name, (scratch, vgprs, static_lds) in mine.items():
        print(name, "scratch", scratch, "vgprs", vgprs, "static LDS", static_lds)
        assert scratch == 0, (name, scratch)
        assert vgprs <= 128, (name, vgprs)   # at least 4 waves per SIMD
        assert static_lds == 0, (name, static_lds)
