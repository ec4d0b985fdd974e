"""Build-time pin of the NUTS step kernel (csrc/nuts_kernel.hip), read from the code objects of the library that was just built
(pathfinder.jl_amd/tools/kernel_resources.py): every instantiation the launcher can take -- column padding 4 .. 64, factor rows staged in
LDS or streamed -- exists exactly once, compiles for gfx950 without scratch and without spills to memory (the definition of
tests/test_hmc_kernel_resources.py: no private segment, no spilled vector register), and its static LDS (the reduction buffers, the three
KPAD-long vectors, the chain's scalars) leaves the 150 KB of staged factor rows inside the 160 KB of a compute unit.  The compiler does
move 2 .. 6 scalar registers into lanes of a vector register (sgpr_spill_count; static HMC's kernel has none): the records', the
block's and the path's addresses are all uniform.  That costs no memory traffic and no scratch; it is printed here and capped at 8."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pathfinder.jl_amd", "tools"))

KPADS = (4, 8, 12, 16, 20, 32, 64)
LDS_LIMIT = 160 * 1024
LDS_RES = 150 * 1024                                            # NT_LDS_RES: pf_hmc_resident's rule
LAUNCHED = [f"pf_nuts_step_kernel<{k}, {r}>(" for k in KPADS for r in ("true", "false")]


@pytest.fixture(scope="module")
def table():
    import kernel_resources as kr
    import pfmi
    pfmi.build()
    return kr.kernel_resources()


@pytest.mark.parametrize("prefix", LAUNCHED)
def test_nuts_step_kernel_has_no_scratch_and_fits_lds(table, prefix):
    hits = [k for k in table if k.startswith(prefix)]
    assert len(hits) == 1, (prefix, hits)
    r = table[hits[0]]
    print("NUTS_KERNEL", hits[0].split("(")[0], "vgpr", r["vgpr_count"], "sgpr to lanes", r["sgpr_spill_count"], "lds", r["group_segment_fixed_size"])
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] <= 8, (hits[0], r)
    kpad = int(prefix.split("<")[1].split(",")[0])
    static = r["group_segment_fixed_size"]
    nred = max(kpad + 4, 24)                                    # the wider of the operator passes' and the decisions' reductions
    assert static >= 8 * (2 * 4 * nred + 3 * kpad), (hits[0], r)
    assert static + (LDS_RES if "true" in prefix else 0) <= LDS_LIMIT, (hits[0], r)
    assert r["vgpr_count"] <= 512, (hits[0], r)                 # 256 threads: one wave per SIMD, all 512 registers (VGPR + AGPR)


def test_no_other_nuts_step_instantiation_exists(table):
    steps = [k for k in table if k.startswith("pf_nuts_step_kernel<")]
    assert len(steps) == len(LAUNCHED), steps


def test_lds_budget_matches_the_source():
    src = open(os.path.join(ROOT, "pathfinder.jl_amd", "csrc", "nuts_kernel.hip")).read()
    assert "#define NT_LDS_RES (150 * 1024)" in src and "#define NT_MAXD 10" in src
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hmc_reference as H
    assert H.LDS_RES == LDS_RES and H.KPADS == KPADS
