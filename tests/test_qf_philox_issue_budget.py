"""Build-time pin of the ELBO scan's block loop after the per-draw Philox rounds left it (profiles/r09_scan_philox.md).

The scan's generator call has the counter (draw, 4 blk + q, 0, 0).  Most of its rounds 1 - 3 depends on the draw alone and is formed
once per batch (`pf_philox_draw_invariants`: the words C, D, E, F per group); one product depends on the block alone and is shared by
the groups of a wave.  A block then issues 9 products per group and 1 shared product: 19 `v_mad_u64_u32` where 23 - 24 were.

All three pinned instantiations ship the full hoist.  Counts come from `pathfinder.jl_amd/tools/qf_issue_count.py`:
- `mad_u64` <= 19, the full hoist's count;
- `valu32` <= the shipped count + 2;
- `vmem` equal to the parent's (the interior trip holds no scratch instruction);
- the MFMA count exact.
The register and scratch pins are those of tests/test_kernel_resources.py, unchanged.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pathfinder.jl_amd", "tools"))

# instantiation -> (mad_u64 cap, shipped valu32, vmem)
SHIPPED = {
    (12, 1, 8, 2): (19, 73, 8),        # config 3/4 (the benchmark)
    (12, 1, 0, 2): (19, 72, 0),        # config 2
    (20, 2, 0, 2): (19, 83, 0),        # config 5
}


@pytest.fixture(scope="module")
def asm():
    import qf_issue_count as qi
    return qi.compile_asm()


@pytest.mark.parametrize("inst", sorted(SHIPPED))
def test_hoisted_block_counts(asm, inst):
    import qf_issue_count as qi
    mad, valu32, vmem = SHIPPED[inst]
    r = qi.steady_counts(asm, *inst)
    assert r["mfma4"] == qi.mfma4_per_block(*inst), (inst, r)
    assert r["mad_u64"] <= mad, (inst, r["mad_u64"])
    assert r["valu32"] <= valu32 + 2, (inst, r["valu32"])
    assert r["vmem"] == vmem, (inst, r["vmem"])


@pytest.mark.parametrize("inst", sorted(SHIPPED))
def test_interior_trip_has_no_scratch_access(asm, inst):
    import qf_issue_count as qi
    blocks = qi.parse_blocks(qi.kernel_lines(asm, qi.mangled(*inst)))
    trip = qi.steady_trip(blocks, qi.steady_counts(asm, *inst)["header"])
    assert not [s for s in trip if s.startswith("scratch_")]
