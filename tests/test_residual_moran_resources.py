"""Resources of bl_residual_moran's kernels, read from the built library's code objects as tests/test_kernel_resources.py reads them.

Every kernel runs without scratch, within 128 vector registers (at least 4 waves per SIMD) and without LDS: the sums over sites are the
wave's shuffle tree and a workspace of wave partials, nothing goes through shared memory.  What occupies the vector registers: the
values and the site kernel hold one cell's conditional, its two generators and four float64 values; the gather holds per field the mean,
the site's own value and the two accumulators of its row (16 doubles) next to a neighbour's 32-byte record; the two kernels that add
the waves' partials hold eight iterations' loads ahead of the additions.  Read from the build this test came with: values 81, means
72, gather 78, finish 70, site 60."""
import re

from test_kernel_resources import kernel_metadata, needs_toolchain

KERNELS = ("values", "means", "gather", "finish", "site")


@needs_toolchain
def test_residual_moran_kernels_stay_in_registers_without_lds(tmp_path_factory):
    meta = kernel_metadata(str(tmp_path_factory.getbasetemp()))
    mine = {n: v for n, v in meta.items() if re.match(r"_Z\d+bl_residual_moran_", n)}
    assert sorted(re.match(r"_Z\d+bl_residual_moran_([a-z]+)_kernel", n).group(1) for n in mine) == sorted(KERNELS), sorted(mine)
    for name, (scratch, vgprs, static_lds) in mine.items():
        print(name, "scratch", scratch, "vgprs", vgprs, "of 128", "static LDS", static_lds)
        assert scratch == 0, (name, scratch)
        assert vgprs <= 128, (name, vgprs)
        assert static_lds == 0, (name, static_lds)
