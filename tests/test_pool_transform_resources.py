"""Build-time pin of the pool-transform kernels (csrc/pool_transform_kernels.hip), read from the code objects of the library that
was just built (pathfinder.jl_amd/tools/kernel_resources.py): no scratch and no LDS anywhere -- the pass keeps a column's sums in
registers and adds the lanes on the DPP path --, and every instantiation the launcher takes keeps the VGPR count of the shipped build
(SHIPPED below) within HEADROOM registers: a ceiling per instantiation, so that a register regression shows long before the wave
reaches 256 registers and with that one wave per SIMD.  (224: the rank-16 family at V = 1, 4 columns x 17 sums.)"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pathfinder.jl_amd", "tools"))

FAMILIES = ((0, 0), (1, 0), (1, 8), (1, 16), (2, 0))           # (TGT, RPAD)
HEADROOM = 8
SHIPPED = {"pf_pool_transform_rows_kernel<0, 0, 1>(": 40, "pf_pool_transform_rows_kernel<0, 0, 2>(": 52,
           "pf_pool_transform_rows_kernel<1, 0, 1>(": 54, "pf_pool_transform_rows_kernel<1, 0, 2>(": 70,
           "pf_pool_transform_rows_kernel<1, 8, 1>(": 139, "pf_pool_transform_rows_kernel<1, 8, 2>(": 171,
           "pf_pool_transform_rows_kernel<1, 16, 1>(": 224,
           "pf_pool_transform_rows_kernel<2, 0, 1>(": 82, "pf_pool_transform_rows_kernel<2, 0, 2>(": 94,
           "pf_pool_transform_cols_kernel<0, 0>(": 14, "pf_pool_transform_cols_kernel<1, 0>(": 16, "pf_pool_transform_cols_kernel<1, 8>(": 33,
           "pf_pool_transform_cols_kernel<1, 16>(": 52, "pf_pool_transform_cols_kernel<2, 0>(": 42, "pf_pool_transform_ratio_kernel(": 8}
LAUNCHED = ([f"pf_pool_transform_rows_kernel<{t}, {r}, {v}>(" for t, r in FAMILIES for v in (1, 2) if not (r == 16 and v == 2)]
            + [f"pf_pool_transform_cols_kernel<{t}, {r}>(" for t, r in FAMILIES] + ["pf_pool_transform_ratio_kernel("])


@pytest.fixture(scope="module")
def table():
    import kernel_resources as kr
    import pfmi
    pfmi.build()
    return kr.kernel_resources()


@pytest.mark.parametrize("prefix", LAUNCHED)
def test_pool_transform_kernels_stay_in_registers(table, prefix):
    hits = [k for k in table if k.startswith(prefix)]
    assert len(hits) == 1, (prefix, hits)
    r = table[hits[0]]
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (hits[0], r)
    assert r["group_segment_fixed_size"] == 0, (hits[0], r)
    assert r["vgpr_count"] <= min(SHIPPED[prefix] + HEADROOM, 256), (hits[0], r, SHIPPED[prefix])


def test_every_launched_instantiation_has_a_ceiling():
    assert set(SHIPPED) == set(LAUNCHED)
