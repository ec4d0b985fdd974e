"""Build-time pin of the fused NUTS kernel (csrc/nuts_fused_kernel.hip), read from the code objects of the library that was just built
(pathfinder.jl_amd/tools/kernel_resources.py, through tests/chain_kernel_resources.py): every instantiation the launcher can take --
column padding 4 .. 64 x factor rows staged in LDS or streamed x {funnel, Gaussian family with rank padding 0, 8, 16}: 56 -- compiles
for gfx950 without scratch and without a spilled vector register, holds the LDS of its reductions (the widest of KPAD + 4, the 24 dot
products of a leaf's decisions and RPAD + 4 values), the three KPAD-long vectors and G's copy, and leaves the HM_LDS_RES bytes of staged
factor rows inside the 160 KB of a compute unit.  Scalar registers moved into lanes of a vector register are printed, not capped, as for
the fused static-HMC kernel: the loop keeps the kernel's arguments live across its trips, and a lane move costs no memory traffic."""
import os

import pytest

import chain_kernel_resources as ckr
from chain_kernel_resources import KPADS, LDS_LIMIT, LDS_RES

TARGETS = (-1, 0, 8, 16)                                        # HM_TG_FUNNEL, then the Gaussian family's rank paddings
LAUNCHED = [(k, r, t) for k in KPADS for r in ("true", "false") for t in TARGETS]


@pytest.fixture(scope="module")
def table():
    return ckr.built_table()


@pytest.mark.parametrize("kpad,res,tg", LAUNCHED)
def test_fused_kernel_has_no_scratch_no_spills_and_fits_lds(table, kpad, res, tg):
    prefix = f"pf_nuts_fused_kernel<{kpad}, {res}, {tg}>("
    hits = [k for k in table if k.startswith(prefix)]
    assert len(hits) == 1, (prefix, hits)
    r = table[hits[0]]
    print("NUTS_FUSED_KERNEL", hits[0].split("(")[0], "vgpr", r["vgpr_count"], "agpr", r["agpr_count"], "sgpr", r["sgpr_count"], "sgpr to lanes",
          r["sgpr_spill_count"], "lds", r["group_segment_fixed_size"])
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (hits[0], r)
    rpad = tg if tg > 0 else 0
    nred = max(kpad + 4, 24, rpad + 4)
    static = r["group_segment_fixed_size"]
    assert static >= 8 * (2 * 4 * nred + 3 * kpad + rpad * rpad), (hits[0], r)
    assert static + (LDS_RES if res == "true" else 0) <= LDS_LIMIT, (hits[0], r)
    assert r["vgpr_count"] <= 512, (hits[0], r)                 # 256 threads: one wave per SIMD, all 512 registers (VGPR + AGPR)


def test_every_instantiation_is_built_once_and_the_cap_is_stated_once(table):
    assert len([k for k in table if k.startswith("pf_nuts_fused_kernel<")]) == len(LAUNCHED) == 56
    src = ckr.budget_source()
    assert src.count("#define HM_FUSED_ROUNDS 1024") == 1 and src.count("#define HM_FUSED_ROUNDS") == 1
    import nuts_fused_reference as NF
    assert NF.ROUNDS_CAP == 1024
    csrc = os.path.join(ckr.ROOT, "pathfinder.jl_amd", "csrc")
    for name in ("nuts_fused_kernel.hip", "api_nuts_fused.hip", "nuts_kernel.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert "#define HM_LDS_RES" not in text and "#define HM_NT" not in text and "#define HM_FUSED_ROUNDS" not in text, name
