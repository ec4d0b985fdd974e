"""Build-time pin of the ELBO scan's per-batch draw finish (pathfinder.jl_amd/csrc/elbo_qf_kernel.hip, "finish the 16 draws of each group
in registers"), read from the compiler's gfx950 assembly by pathfinder.jl_amd/tools/qf_issue_count.py (`finish_counts`: the kernel's text
from the end of the publish step to `s_endpgm`).

All eight waves of a workgroup reach the finish together, so its latency is wall-clock time of every batch.  The finish reads the A
operands of T, M, Nn and G once per batch, in one flight in front of the chains, runs the chains of a wave's groups in lockstep, and at
KC <= 12 uses one 4x4x4 MFMA per 4 x 4 tile of a matrix.  What this file pins, as upper bounds, are the counts of the build that was
measured (profiles/r12_scan_epilogue.md): the MFMAs per group are what the products need, and hardly any LDS read or wait sits between
the first and the last MFMA of the wave's finish.  Before round 12 the headline instantiation had 11 16x16x4 MFMAs, 15 LDS read
instructions, 14.5 `s_waitcnt` (12 of them inside the chains) and 68 wait states per group.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pathfinder.jl_amd", "tools"))

# instantiation -> (MFMA16, MFMA4, LDS read instructions, scratch loads, waits inside the chains, LDS reads inside the chains), per group
PINS = {
    (12, 1, 8, 2): (0, 28, 10, 0.5, 5.5, 2),
    (12, 1, 0, 2): (0, 18, 6, 0, 1, 1.5),
    (20, 2, 0, 2): (20, 0, 10, 6, 0.5, 1.5),
}


@pytest.fixture(scope="module")
def asm():
    import qf_issue_count as qic
    return qic, qic.compile_asm()


@pytest.mark.parametrize("inst", sorted(PINS))
def test_finish_counts_within_the_measured_build(asm, inst):
    qic, text = asm
    f = qic.finish_counts(text, *inst)["per_group"]
    m16, m4, lds, scr, wic, ric = PINS[inst]
    nt, tr = inst[0] // 4, inst[2] // 4
    if m4:                                                       # one MFMA per 4 x 4 tile: T and M (nt x nt), Nn (tr x nt), G (tr x tr)
        assert m4 == 2 * nt * nt + tr * nt + tr * tr
    assert f["mfma16"] == m16 and f["mfma4"] == m4, f
    assert f["lds_reads"] <= lds and f["scratch_loads"] <= scr, f
    assert f["waits_in_chain"] <= wic and f["reads_in_chain"] <= ric, f
