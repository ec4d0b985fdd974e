"""Build-time pin of the NUTS step kernel (csrc/nuts_kernel.hip), read from the code objects of the library that was just built
(pathfinder.jl_amd/tools/kernel_resources.py): every instantiation the launcher can take -- column padding 4 .. 64, factor rows staged in
LDS or streamed -- exists exactly once, compiles for gfx950 without scratch and without spills to memory (the definition of
tests/test_hmc_kernel_resources.py: no private segment, no spilled vector register), keeps its waves per SIMD, and its static LDS (the
reduction buffers, the three KPAD-long vectors, the chain's scalars) leaves the 150 KB of staged factor rows inside the 160 KB of a compute
unit.  The compiler does move 2 .. 6 scalar registers into lanes of a vector register (sgpr_spill_count; static HMC's kernel has none): the
records', the block's and the path's addresses are all uniform.  That costs no memory traffic and no scratch; it is printed here, capped at
8 and at what the instantiation had before the passes were shared (the check itself: tests/chain_kernel_resources.py)."""
import os

import pytest

import chain_kernel_resources as ckr
from chain_kernel_resources import KPADS, LDS_RES

LAUNCHED = [f"pf_nuts_step_kernel<{k}, {r}>(" for k in KPADS for r in ("true", "false")]


@pytest.fixture(scope="module")
def table():
    return ckr.built_table()


@pytest.mark.parametrize("prefix", LAUNCHED)
def test_nuts_step_kernel_has_no_scratch_and_fits_lds(table, prefix):
    kpad, res = prefix.split("<")[1].split(">")[0].split(", ")
    r = ckr.check_instantiation(table, "pf_nuts_step_kernel", int(kpad), res, "NUTS_KERNEL")
    assert r["sgpr_spill_count"] <= 8, (prefix, r)


def test_no_other_nuts_step_instantiation_exists(table):
    steps = [k for k in table if k.startswith("pf_nuts_step_kernel<")]
    assert len(steps) == len(LAUNCHED), steps


def test_lds_budget_matches_the_source():
    src = ckr.budget_source()
    assert src.count("#define HM_LDS_RES (150 * 1024)") == 1
    nuts = open(os.path.join(ckr.ROOT, "pathfinder.jl_amd", "csrc", "nuts_kernel.hip")).read()
    assert '#include "hmc_rows.h"' in nuts and "_LDS_RES (" not in nuts and "#define NT_MAXD 10" in nuts
    import hmc_reference as H
    assert H.LDS_RES == LDS_RES == 150 * 1024 and H.KPADS == KPADS
