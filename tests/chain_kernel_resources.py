"""What the build-time pins of the chain kernels share (tests/test_hmc_kernel_resources.py, test_nuts_kernel_resources.py,
test_adapt_kernel_resources.py): the resource table of the library that was just built, the one statement of the LDS budget in the
source (csrc/hmc_rows.h), and the check every instantiation of pf_hmc_step_kernel, pf_hmc_warm_kernel, pf_nuts_step_kernel and
pf_nuts_warm_kernel has to pass.

BEFORE holds, per instantiation, (vgpr_count, sgpr_spill_count) of the kernels as they were before the two Woodbury passes moved into
hmc_rows.h (commit 5a1c8db, same compiler).  Registers are allocated in steps of 8 and a SIMD has 512 per lane, so an instantiation
runs floor(512 / (ceil(vgpr / 8) * 8)) waves per SIMD; sharing the passes must not cost a wave, nor move more scalar registers into
lanes of a vector register than before (static HMC: none)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pathfinder.jl_amd", "tools"))

KPADS = (4, 8, 12, 16, 20, 32, 64)
LDS_LIMIT = 160 * 1024
LDS_RES = 150 * 1024                                            # HM_LDS_RES
SGPR_TO_LANES_CAP = 8
_T, _F = "true", "false"
BEFORE = {
    "pf_hmc_step_kernel": {(4, _T): (42, 0), (4, _F): (40, 0), (8, _T): (58, 0), (8, _F): (60, 0), (12, _T): (72, 0), (12, _F): (76, 0),
                           (16, _T): (88, 0), (16, _F): (92, 0), (20, _T): (104, 0), (20, _F): (108, 0), (32, _T): (98, 0), (32, _F): (98, 0),
                           (64, _T): (166, 0), (64, _F): (166, 0)},
    "pf_hmc_warm_kernel": {(4, _T): (45, 0), (4, _F): (45, 0), (8, _T): (60, 0), (8, _F): (62, 0), (12, _T): (74, 0), (12, _F): (78, 0),
                           (16, _T): (90, 0), (16, _F): (94, 0), (20, _T): (106, 0), (20, _F): (110, 0), (32, _T): (98, 0), (32, _F): (98, 0),
                           (64, _T): (166, 0), (64, _F): (166, 0)},
    "pf_nuts_step_kernel": {(4, _T): (127, 6), (4, _F): (127, 2), (8, _T): (127, 6), (8, _F): (127, 2), (12, _T): (127, 5), (12, _F): (127, 2),
                            (16, _T): (127, 4), (16, _F): (127, 2), (20, _T): (127, 5), (20, _F): (127, 2), (32, _T): (127, 4), (32, _F): (127, 2),
                            (64, _T): (189, 4), (64, _F): (189, 2)},
    "pf_nuts_warm_kernel": {(4, _T): (127, 6), (4, _F): (127, 2), (8, _T): (127, 6), (8, _F): (127, 2), (12, _T): (127, 6), (12, _F): (127, 2),
                            (16, _T): (127, 8), (16, _F): (127, 2), (20, _T): (127, 6), (20, _F): (127, 4), (32, _T): (127, 4), (32, _F): (127, 4),
                            (64, _T): (187, 6), (64, _F): (187, 4)},
}


def waves_per_simd(vgpr):
    return 512 // (-(-vgpr // 8) * 8)


def built_table():
    import kernel_resources as kr
    import pfmi
    pfmi.build()
    return kr.kernel_resources()


def budget_source():
    """the one file that states the chain kernels' thread count and LDS budget"""
    return open(os.path.join(ROOT, "pathfinder.jl_amd", "csrc", "hmc_rows.h")).read()


def check_instantiation(table, name, kpad, res, tag):
    """`name`<kpad, res> exists exactly once, has no scratch and no spilled vector register, fits the LDS, keeps the waves per SIMD and
    the scalar registers in lanes within what it had before; returns its resources"""
    prefix = f"{name}<{kpad}, {res}>("
    hits = [k for k in table if k.startswith(prefix)]
    assert len(hits) == 1, (prefix, hits)
    r = table[hits[0]]
    print(tag, hits[0].split("(")[0], "vgpr", r["vgpr_count"], "sgpr", r["sgpr_count"], "sgpr to lanes", r["sgpr_spill_count"], "lds",
          r["group_segment_fixed_size"])
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (hits[0], r)
    vgpr0, lanes0 = BEFORE[name][(kpad, res)]
    assert r["sgpr_spill_count"] <= min(lanes0, SGPR_TO_LANES_CAP), (hits[0], r, lanes0)
    assert waves_per_simd(r["vgpr_count"]) >= waves_per_simd(vgpr0), (hits[0], r, vgpr0)
    static = r["group_segment_fixed_size"]
    nred = max(kpad + 4, 24) if "nuts" in name else kpad + 4   # NUTS: the wider of the operator passes' and the decisions' reductions
    assert static >= 8 * (2 * 4 * nred + 3 * kpad), (hits[0], r)                 # the ping-pong reduction buffers, sHead, sZ, sTv
    assert static + (LDS_RES if res == "true" else 0) <= LDS_LIMIT, (hits[0], r)
    assert r["vgpr_count"] <= 512, (hits[0], r)                 # 256 threads: one wave per SIMD, all 512 registers (VGPR + AGPR)
    return r
