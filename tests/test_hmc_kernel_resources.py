"""Build-time pin of the HMC step kernel (csrc/hmc_kernel.hip), read from the code objects of the library that was just built
(pathfinder.jl_amd/tools/kernel_resources.py): every instantiation the launcher can take -- column padding 4 .. 64, factor rows staged
in LDS or streamed -- compiles for gfx950 without scratch and without spills, and its static LDS (the reduction buffers and the three
KPAD-long vectors) leaves the HM_LDS_RES bytes of staged factor rows inside the 160 KB of a compute unit."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pathfinder.jl_amd", "tools"))

KPADS = (4, 8, 12, 16, 20, 32, 64)
LDS_LIMIT = 160 * 1024
LDS_RES = 150 * 1024                                            # HM_LDS_RES
LAUNCHED = [f"pf_hmc_step_kernel<{k}, {r}>(" for k in KPADS for r in ("true", "false")]


@pytest.fixture(scope="module")
def table():
    import kernel_resources as kr
    import pfmi
    pfmi.build()
    return kr.kernel_resources()


@pytest.mark.parametrize("prefix", LAUNCHED)
def test_hmc_step_kernel_has_no_scratch_and_fits_lds(table, prefix):
    hits = [k for k in table if k.startswith(prefix)]
    assert len(hits) == 1, (prefix, hits)
    r = table[hits[0]]
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (hits[0], r)
    kpad = int(prefix.split("<")[1].split(",")[0])
    static = r["group_segment_fixed_size"]
    assert static >= 8 * (2 * 4 * (kpad + 4) + 3 * kpad), (hits[0], r)           # the ping-pong reduction buffers, sHead, sZ, sTv
    assert static + (LDS_RES if "true" in prefix else 0) <= LDS_LIMIT, (hits[0], r)
    assert r["vgpr_count"] <= 512, (hits[0], r)                 # 256 threads: one wave per SIMD, all 512 registers (VGPR + AGPR)


def test_lds_budget_matches_the_source():
    src = open(os.path.join(ROOT, "pathfinder.jl_amd", "csrc", "hmc_kernel.hip")).read()
    assert "#define HM_LDS_RES (150 * 1024)" in src
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hmc_reference as H
    assert H.LDS_RES == LDS_RES and H.KPADS == KPADS
