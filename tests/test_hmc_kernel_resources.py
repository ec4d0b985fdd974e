"""Build-time pin of the HMC step kernel (csrc/hmc_kernel.hip), read from the code objects of the library that was just built
(pathfinder.jl_amd/tools/kernel_resources.py): every instantiation the launcher can take -- column padding 4 .. 64, factor rows staged
in LDS or streamed -- compiles for gfx950 without scratch and without spills, moves no scalar register into a lane, keeps its waves per
SIMD, and its static LDS (the reduction buffers and the three KPAD-long vectors) leaves the HM_LDS_RES bytes of staged factor rows
inside the 160 KB of a compute unit (the check itself: tests/chain_kernel_resources.py)."""
import os

import pytest

import chain_kernel_resources as ckr
from chain_kernel_resources import KPADS, LDS_RES

LAUNCHED = [f"pf_hmc_step_kernel<{k}, {r}>(" for k in KPADS for r in ("true", "false")]


@pytest.fixture(scope="module")
def table():
    return ckr.built_table()


@pytest.mark.parametrize("prefix", LAUNCHED)
def test_hmc_step_kernel_has_no_scratch_and_fits_lds(table, prefix):
    kpad, res = prefix.split("<")[1].split(">")[0].split(", ")
    r = ckr.check_instantiation(table, "pf_hmc_step_kernel", int(kpad), res, "HMC_KERNEL")
    assert r["sgpr_spill_count"] == 0, (prefix, r)


def test_lds_budget_matches_the_source():
    src = ckr.budget_source()
    assert src.count("#define HM_LDS_RES (150 * 1024)") == 1 and src.count("#define HM_NT 256") == 1
    hmc = open(os.path.join(ckr.ROOT, "pathfinder.jl_amd", "csrc", "hmc_kernel.hip")).read()
    assert '#include "hmc_rows.h"' in hmc and "#define HM_LDS_RES" not in hmc and "#define HM_NT" not in hmc
    import hmc_reference as H
    assert H.LDS_RES == LDS_RES == 150 * 1024 and H.KPADS == KPADS
