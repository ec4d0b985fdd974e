"""Build-time pin of the PSIS workgroup kernels after their body moved into one device function (csrc/psis_kernels.hip:
pf_psis_segment): the two pf_psis_kernel instantiations and pf_psis_runs_kernel, which all inline it, read from the code objects of the
library that was just built (pathfinder.jl_amd/tools/kernel_resources.py).  A 1024-thread workgroup is 4 waves per SIMD, so 128 VGPRs
is where the kernel stops launching at all; the shipped build has 120 in all three and no scratch.  LDS: the 4096-entry tail (48 KB) plus
the selection state; 53 248 B keeps three workgroups inside a CU's 160 KB (the shipped build: 52 664 / 52 792 B)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pathfinder.jl_amd", "tools"))

KERNELS = ("pf_psis_kernel<false>(", "pf_psis_kernel<true>(", "pf_psis_runs_kernel(")


@pytest.fixture(scope="module")
def table():
    import kernel_resources as kr
    import pfmi
    pfmi.build()
    return kr.kernel_resources()


@pytest.mark.parametrize("prefix", KERNELS)
def test_psis_workgroup_kernels_fit_a_1024_thread_workgroup_without_scratch(table, prefix):
    hits = [k for k in table if k.startswith(prefix)]
    assert len(hits) == 1, (prefix, hits)
    r = table[hits[0]]
    assert r["vgpr_count"] <= 128, (hits[0], r)
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (hits[0], r)
    assert r["group_segment_fixed_size"] <= 53248, (hits[0], r)
    assert r["max_flat_workgroup_size"] == 1024, (hits[0], r)
