"""Build-time pin of the chain-diagnostics kernels (csrc/chain_diag_kernels.hip), read from the code objects of the library that was just
built (pathfinder.jl_amd/tools/kernel_resources.py): every kernel pfmi_chain_diagnostics launches compiles for gfx950 without scratch
and without spills, and the static LDS of the tile-sort and the counting kernel is their one tile of CD_TILE doubles."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pathfinder.jl_amd", "tools"))

LAUNCHED = ["pf_cd_transpose_kernel(", "pf_cd_moments_kernel(", "pf_cd_tilesort_kernel<false>(", "pf_cd_tilesort_kernel<true>(",
            "pf_cd_rank_kernel<false>(", "pf_cd_rank_kernel<true>(", "pf_cd_ess_kernel(",
            "pf_cd_final_kernel("]
TILE = 2048


@pytest.fixture(scope="module")
def table():
    import kernel_resources as kr
    import pfmi
    pfmi.build()
    return kr.kernel_resources()


@pytest.mark.parametrize("prefix", LAUNCHED)
def test_chain_diag_kernels_have_no_scratch(table, prefix):
    hits = [k for k in table if k.startswith(prefix)]
    assert len(hits) == 1, (prefix, hits)
    r = table[hits[0]]
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (hits[0], r)
    if "rank" in prefix or "tilesort" in prefix:
        assert r["group_segment_fixed_size"] == 8 * TILE, (hits[0], r)
    assert r["group_segment_fixed_size"] <= 64 * 1024, (hits[0], r)


def test_tile_matches_the_source_and_the_reference():
    src = open(os.path.join(ROOT, "pathfinder.jl_amd", "csrc", "chain_diag_kernels.hip")).read()
    assert "#define CD_TILE %d " % TILE in src
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import chain_diag_reference as R
    assert R.TILE == TILE
