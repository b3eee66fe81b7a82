"""Resources of bl_species_richness' kernels, read from the built library's code objects as tests/test_kernel_resources.py reads them.

The recursion's pmf is a register array indexed by the unrolled loops' own counters only, so every instantiation runs without scratch
and without LDS.  What occupies the vector registers, two per float64:

* area kernel, capacity class CAP: the pmf's CAP + 1 entries, the 16 staged covariates, the weight, and the block of four terms a
  reduction step holds;
* site kernel with the pmf, class CAP: the pmf's CAP + 1 entries AND their CAP + 1 accumulators over the draws, the accumulator of E,
  the 16 staged covariates;
* site kernel without the pmf and the finish kernel (32 partials loaded ahead of the additions): no recursion.

The caps: the 8-species class and the kernels without a recursion leave at least 4 waves per SIMD (<= 128); the 16- and 32-species
classes get what the arrays above need -- 2 (CAP + 1) for the area side, 4 (CAP + 1) for the site side -- plus the 64 registers the
8-species class is seen to use beside its arrays, rounded up to the allocation granule of 8: no instantiation may spend more than its
arrays explain.  Read from the build this test came with: area 87 / 83 / 115 (classes 8 / 16 / 32, caps 128 / 104 / 136), site 95 / 104 /
165 (caps 128 / 136 / 200), site without the pmf 32, finish 104; so the 32-species site kernel runs 3 waves per SIMD, the 32-species area
kernel and the 16-species site kernel 4, everything else 4 or more."""
import re

from test_kernel_resources import kernel_metadata, needs_toolchain


def _granule(v):
    return (v + 7) // 8 * 8


BESIDE = 64   # covariates, weight, addresses, a block of terms, the transcendental's temporaries
CAPS = {
    ("area", 8): 128, ("area", 16): _granule(2 * 17 + BESIDE), ("area", 32): _granule(2 * 33 + BESIDE),
    ("site", 0): 128, ("site", 8): 128, ("site", 16): _granule(4 * 17 + BESIDE), ("site", 32): _granule(4 * 33 + BESIDE),
    ("finish", None): 128,
}


def _which(name):
    """The mangled kernel name -> (side, capacity class)."""
    if "finish" in name:
        return ("finish", None)
    side = "area" if "area_kernel" in name else "site"
    cap = int(re.search(r"kernelILi(\d+)", name).group(1))
    return (side, cap)


@needs_toolchain
def test_species_richness_kernels_stay_in_registers_without_lds(tmp_path_factory):
    meta = kernel_metadata(str(tmp_path_factory.getbasetemp()))
    mine = {n: v for n, v in meta.items() if re.match(r"_Z\d+bl_species_richness_", n)}
    assert sorted(_which(n) for n in mine if "finish" not in n) == sorted(k for k in CAPS if k[0] != "finish"), sorted(mine)
    assert sum("finish" in n for n in mine) == 1, sorted(mine)
    for name, (scratch, vgprs, static_lds) in mine.items():
        cap = CAPS[_which(name)]
        print(name, "scratch", scratch, "vgprs", vgprs, "of", cap, "static LDS", static_lds)
        assert scratch == 0, (name, scratch)
        assert static_lds == 0, (name, static_lds)
        assert vgprs <= cap, (name, vgprs, cap)
