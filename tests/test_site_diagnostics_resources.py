"""Resources of bl_site_diagnostics' kernels, read from the built library's code objects as tests/test_kernel_resources.py reads them: a
pass over the lags keeps BL_SD_LAGS = 32 float64 accumulators and a ring of as many trailing values next to the cell's staged covariates,
all of it at static register indices -- a ring in scratch memory would be read 32 times per draw, chain and pass."""
import re

from test_kernel_resources import kernel_metadata, needs_toolchain


@needs_toolchain
def test_site_diagnostics_kernels_keep_ring_and_accumulators_in_registers(tmp_path_factory):
    meta = kernel_metadata(str(tmp_path_factory.getbasetemp()))
    mine = {n: v for n, v in meta.items() if re.match(r"_Z\d+bl_site_diagnostics_(?:psi|prob)_kernelILin?\d+EE", n)}
    # both sites, each for 0 .. 4 covariates and for any number (-1)
    forms = sorted((re.search(r"diagnostics_(psi|prob)_", n).group(1), int(re.search(r"kernelILi(n?\d+)E", n).group(1).replace("n", "-"))) for n in mine)
    assert forms == sorted((s, k) for s in ("psi", "prob") for k in (-1, 0, 1, 2, 3, 4)), sorted(mine)
    for name, (scratch, vgprs, static_lds) in mine.items():
        assert scratch == 0, (name, scratch)
        assert vgprs <= 192, (name, vgprs)   # 2 x 32 float64 = 128 registers are the design; 152 - 175 as built
        assert static_lds == 0, (name, static_lds)
