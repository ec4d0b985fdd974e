"""Build-time pin of the ELBO scan's block loop after the linear-term fold and the clamp-free table look-up.

Two cuts of the interior block's non-MFMA issue (profiles/r08_scan_fold.md):
- The linear term 2 a c s z is folded into the B operand of the A3 MFMAs: one fma gives both that operand and the factor of the
  scalar sum, so each row of each group loses an f64 add.
- The inverse-CDF interval index is one `v_bfe_u32` instead of a shift and a `v_max_u32` clamp. The LDS guards on both sides of
  the table keep every index inside the allocation.

Counts come from `pathfinder.jl_amd/tools/qf_issue_count.py`. The MFMA counts are exact; the other counts are caps.
"""
import os
import struct
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pathfinder.jl_amd", "tools"))

# instantiation -> {class: cap per block}
CAPS = {
    (12, 1, 8, 2): {"valu_f64": 56, "valu32": 80, "mov_b64": 0},       # config 3/4 (the benchmark)
    (12, 1, 0, 2): {"valu_f64": 48, "valu32": 80, "mov_b64": 0},       # config 2
    # the register-lean body keeps the unfused operand (see FOLD in the kernel); it gets the look-up cut only
    (20, 2, 0, 2): {"valu_f64": 56, "valu32": 90, "mov_b64": 0},       # config 5
}


@pytest.fixture(scope="module")
def asm():
    import qf_issue_count as qi
    return qi.compile_asm()


@pytest.mark.parametrize("inst", sorted(CAPS))
def test_folded_block_counts(asm, inst):
    import qf_issue_count as qi
    r = qi.steady_counts(asm, *inst)
    assert r["mfma4"] == qi.mfma4_per_block(*inst), (inst, r)
    over = {k: (r[k], v) for k, v in CAPS[inst].items() if r[k] > v}
    assert not over, f"pf_elbo_qf_kernel<{inst}>: per-block counts above their caps (count, cap): {over}"


def test_lookup_is_one_bfe_without_clamp(asm):
    """the steady trip forms each of its 8 table indices with v_bfe_u32 and has no v_max_u32"""
    import qf_issue_count as qi
    blocks = qi.parse_blocks(qi.kernel_lines(asm, qi.mangled(12, 1, 8, 2)))
    trip = qi.steady_trip(blocks, qi.steady_counts(asm, 12, 1, 8, 2)["header"])
    ops = [s.split()[0] for s in trip]
    assert sum(o.startswith("v_bfe_u32") for o in ops) >= 8
    assert not any(o.startswith("v_max_u32") for o in ops)


def _hdr_int(name):
    with open(os.path.join(ROOT, "pathfinder.jl_amd", "csrc", "pfmi_icdftab.h")) as f:
        for line in f:
            if line.startswith(f"#define {name} "):
                return int(line.split()[2])
    raise KeyError(name)


def test_bfe_index_keeps_every_word_inside_the_guards():
    """Host model of pf_icdf_issue_bfe against pf_icdf_issue_adj.

    Every 31-bit magnitude gets a slot in [-FRONT, NENT + BEHIND). Every magnitude the LDS copy serves gets the same slot as before.
    One word per interval and every exponent are enough: the index depends only on the top bits of the double."""
    B, IDX0, NB = _hdr_int("PF_ICDF_B"), _hdr_int("PF_ICDF_IDX0"), _hdr_int("PF_ICDF_NB_LDS")
    nent = NB << B
    slot0 = IDX0 - (nent - 1)
    base = slot0 & 1023
    front, behind = base, 1024 - base - nent
    assert (front, behind) == (352, 64)           # the guards the scan reserves (QF_MIN_FRONT, qf_lds_bytes)

    def hi(m):
        return struct.unpack("<Q", struct.pack("<d", float(m)))[0] >> 32

    mags = {0}
    for e in range(31):
        for k in range(1 << B):
            m = (1 << e) + ((k << e) >> B)
            mags.update({m, min(m + 1, (1 << 31) - 1)})
    mags.add((1 << 31) - 1)
    for m in sorted(mags):
        h = hi(m)
        slot = ((h >> (20 - B)) & 1023) - base
        assert -front <= slot < nent + behind, m
        if m >= 1 << (31 - NB):
            assert slot == (h >> (20 - B)) - slot0 and 0 <= slot < nent, m
