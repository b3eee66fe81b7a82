"""Resources of bl_site_summary's kernels, read from the built library's code objects as tests/test_kernel_resources.py reads them: the
select keeps a counter and a candidate per rank (up to BL_SUMMARY_MAX_RANKS = 16 of each) next to the cell's staged covariates, all of
it in registers -- a counter array in scratch memory would be touched once per draw, rank and pass."""
import re

from biolith_amd import _ffi
from test_kernel_resources import kernel_metadata, needs_toolchain


@needs_toolchain
def test_site_summary_kernels_keep_their_counters_in_registers(tmp_path_factory):
    meta = kernel_metadata(str(tmp_path_factory.getbasetemp()))
    mine = {n: v for n, v in meta.items() if re.match(r"_Z\d+bl_site_summary_(?:psi|prob)_kernelILi\d+ELin?\d+EE", n)}
    # both sites, each with 0 (mean and sd alone), 4, 8 and 16 counters, each of those for 0 .. 4 covariates and for any number (-1)
    forms = sorted((re.search(r"summary_(psi|prob)_", n).group(1),) + tuple(int(g.replace("n", "-")) for g in re.search(r"kernelILi(\d+)ELi(n?\d+)E", n).groups())
                   for n in mine)
    assert forms == sorted((s, r, k) for s in ("psi", "prob") for r in (0, 4, 8, _ffi.SUMMARY_MAX_RANKS) for k in (-1, 0, 1, 2, 3, 4)), sorted(mine)
    for name, (scratch, vgprs, static_lds) in mine.items():
        assert scratch == 0, (name, scratch)
        assert vgprs <= 128, (name, vgprs)   # at least 4 waves per SIMD
        assert static_lds == 0, (name, static_lds)
