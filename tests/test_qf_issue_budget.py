"""Build-time pin of the ELBO scan's per-block instruction issue (the steady-state block loop of `pf_elbo_qf_kernel`).

The scan is issue bound: on gfx950 the f64 MFMA co-issues with nothing, so every non-MFMA instruction of the interior block adds its
full issue cost to the kernel's time (profiles/r02_coissue_microbench.txt).  Round 7 peeled the first / second / last block out of
the interior loop: the interior trip lost 20 loop-carried `v_mov_b64` accumulator copies, 12 waits, 6 scalar instructions and 2
branches per block at <12, 1, 8, 2> (profiles/r07_scan_issue.md).  Those savings depend on how the compiler lays out the loop; a source
change or a toolchain upgrade that puts instructions back into the interior block fails here, on the CPU, before anybody measures.

Counts come from `pathfinder.jl_amd/tools/qf_issue_count.py` (the library's flags, `hipcc -S`); bounds are the round-7 build's values
plus a little slack for scheduling noise, the MFMA counts exact.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pathfinder.jl_amd", "tools"))

# instantiation -> (why, {class: max per block}, max estimated non-MFMA issue cycles per block)
BUDGET = {
    (12, 1, 8, 2): ("config 3/4 scan (the benchmark)",
                    {"mov_b64": 0, "valu_f64": 64, "mad_u64": 23, "valu32": 88, "lds": 28, "vmem": 8, "salu": 6, "nop_cycles": 8,
                     "waitcnt": 14, "branch": 4}, 975),
    (12, 1, 0, 2): ("config 2 scan (diagonal Gaussian)",
                    {"mov_b64": 0, "valu_f64": 56, "mad_u64": 23, "valu32": 87, "lds": 26, "vmem": 0, "salu": 6, "nop_cycles": 8,
                     "waitcnt": 8, "branch": 4}, 890),
    # (the register-lean body keeps the round-6 loop, see the kernel: pinned as it is)
    (20, 2, 0, 2): ("config 5 scan (funnel, J = 10, factor streamed): register-lean body",
                    {"mov_b64": 0, "valu_f64": 56, "mad_u64": 24, "valu32": 98, "lds": 30, "vmem": 0, "salu": 22, "nop_cycles": 17,
                     "waitcnt": 18, "branch": 15}, 1000),
}


@pytest.fixture(scope="module")
def asm():
    import qf_issue_count as qi
    return qi.compile_asm()


@pytest.mark.parametrize("inst", sorted(BUDGET))
def test_steady_block_issue_budget(asm, inst):
    import qf_issue_count as qi
    why, caps, cyc = BUDGET[inst]
    r = qi.steady_counts(asm, *inst)
    name = f"pf_elbo_qf_kernel<{', '.join(map(str, inst))}> ({why})"
    assert r["mfma4"] == qi.mfma4_per_block(*inst), (name, r)       # the contraction itself: exactly the block's matrix work
    assert r["mfma16"] == 0, f"{name}: the head transform is back in the interior block: {r}"
    over = {k: (r[k], v) for k, v in caps.items() if r[k] > v}
    assert not over, f"{name}: per-block issue above budget (count, budget): {over}"
    assert r["non_mfma_cycles"] <= cyc, f"{name}: ~{r['non_mfma_cycles']:.0f} non-MFMA issue cycles per block > {cyc}"


def test_steady_path_finder_sees_the_special_blocks_as_special(asm):
    """the loop the tool calls steady is the interior one: the first / last block's extras (row clamp, head transform) are not on it"""
    import qf_issue_count as qi
    r = qi.steady_counts(asm, 12, 1, 8, 2)
    assert r["blocks_per_trip"] == 1 and r["mfma16"] == 0
    kl = qi.parse_blocks(qi.kernel_lines(asm, qi.mangled(12, 1, 8, 2)))
    assert sum(s.startswith("v_mfma_f64_16x16x4") for b in kl for s in b[2]) > 0      # ... while the kernel does have them
