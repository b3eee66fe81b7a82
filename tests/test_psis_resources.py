"""Resources of bl_psis_loo's kernels, read from the built library's code objects as tests/test_kernel_resources.py reads them: the
cell's column lives in LDS, so nothing of it may sit in scratch memory, and the static LDS of the per-cell kernel plus the largest column
it is launched with (4 bytes x BL_PSIS_MAX_DRAWS, dynamic) stays far inside the 160 KiB of a workgroup."""
import re

from biolith_amd import _ffi
from test_kernel_resources import kernel_metadata, needs_toolchain


@needs_toolchain
def test_psis_kernels_keep_the_column_out_of_scratch(tmp_path_factory):
    meta = kernel_metadata(str(tmp_path_factory.getbasetemp()))
    mine = {n: v for n, v in meta.items() if re.match(r"_Z\d+bl_psis_(?:loo|transpose)_kernel", n)}
    assert len(mine) == 2, sorted(mine)
    for name, (scratch, vgprs, static_lds) in mine.items():
        assert scratch == 0, (name, scratch)
        assert vgprs <= 128, (name, vgprs)   # at least 4 waves per SIMD
        dynamic = 4 * _ffi.PSIS_MAX_DRAWS if "loo" in name else 0
        assert static_lds + dynamic <= 160 * 1024 // 4, (name, static_lds)   # four workgroups per CU at the cap
