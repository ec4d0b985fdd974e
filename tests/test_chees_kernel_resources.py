"""Build-time pin of the ChEES kernels (csrc/chees_kernel.hip): pf_chees_step_kernel is the step body of csrc/hmc_kernel.hip in its fourth
mode -- all 14 instantiations exist exactly once, none uses scratch or spills a vector register, the static LDS of each leaves the
HM_LDS_RES bytes of staged factor rows inside the 160 KB of a compute unit: the pins of the metric kernels, the body's third mode
(tests/test_metric_kernel_resources.py), and none has fewer workgroups per SIMD or more scalar registers in vector lanes than RECORDED.
The three kernels of the cross-chain
update exist once each and use no scratch.  (That the step, warm and metric kernels did not move is what
tests/test_hmc_kernel_resources.py, test_adapt_kernel_resources.py and test_metric_kernel_resources.py pin.)"""
import pytest

import chain_kernel_resources as ckr
from chain_kernel_resources import KPADS, LDS_LIMIT, LDS_RES

CHEES = [(k, r) for k in KPADS for r in ("true", "false")]
# (vgpr_count, sgpr_spill_count) of every instantiation as this kernel was first built, recorded the way chain_kernel_resources.BEFORE
# records the step and warm kernels': a later change must not cost an instantiation a workgroup per SIMD, nor move more scalar registers
# into lanes of a vector register.  (The argument struct is 14 pointers longer than the warm kernel's, which is what spills; KPAD 32 holds
# 3 and KPAD 64 holds 2 chains per compute unit where the warm kernel holds 5 and 3.)
RECORDED = {(4, "true"): (43, 40), (4, "false"): (41, 30), (8, "true"): (59, 47), (8, "false"): (59, 32), (12, "true"): (73, 70),
            (12, "false"): (75, 34), (16, "true"): (89, 71), (16, "false"): (91, 32), (20, "true"): (105, 70), (20, "false"): (107, 34),
            (32, "true"): (131, 44), (32, "false"): (129, 28), (64, "true"): (169, 44), (64, "false"): (169, 28)}


@pytest.fixture(scope="module")
def table():
    return ckr.built_table()


@pytest.mark.parametrize("kpad,res", CHEES, ids=["%d-%s" % (k, "res" if r == "true" else "stream") for k, r in CHEES])
def test_chees_step_kernel_has_no_scratch_and_fits_lds(table, kpad, res):
    prefix = f"pf_chees_step_kernel<{kpad}, {res}>("
    hits = [k for k in table if k.startswith(prefix)]
    assert len(hits) == 1, (prefix, hits)
    r = table[hits[0]]
    print("CHEES_KERNEL", hits[0].split("(")[0], "vgpr", r["vgpr_count"], "sgpr", r["sgpr_count"], "sgpr to lanes", r["sgpr_spill_count"], "lds",
          r["group_segment_fixed_size"])
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (hits[0], r)
    static = r["group_segment_fixed_size"]
    assert static >= 8 * (2 * 4 * (kpad + 4) + 3 * kpad), (hits[0], r)           # the ping-pong reduction buffers, sHead, sZ, sTv
    assert static + (LDS_RES if res == "true" else 0) <= LDS_LIMIT, (hits[0], r)
    assert r["vgpr_count"] <= 512, (hits[0], r)
    vgpr0, lanes0 = RECORDED[(kpad, res)]
    assert ckr.waves_per_simd(r["vgpr_count"]) >= ckr.waves_per_simd(vgpr0), (hits[0], r, vgpr0)
    assert r["sgpr_spill_count"] <= lanes0, (hits[0], r, lanes0)
    # (a workgroup is one chain: 4 waves, one per SIMD.  Workgroups per compute unit, printed beside the warm kernel's, only matter once
    # more chains than compute units are resident)
    warm = [k for k in table if k.startswith(f"pf_hmc_warm_kernel<{kpad}, {res}>(")]
    print("CHEES_KERNEL chains per CU", ckr.waves_per_simd(r["vgpr_count"]), "warm kernel", ckr.waves_per_simd(table[warm[0]]["vgpr_count"]))


def test_no_other_chees_step_instantiation_exists(table):
    assert len([k for k in table if k.startswith("pf_chees_step_kernel<")]) == 2 * len(KPADS)


@pytest.mark.parametrize("name", ("pf_chees_mean_kernel", "pf_chees_sums_kernel", "pf_chees_scalar_kernel"))
def test_update_kernels_use_no_scratch(table, name):
    hits = [k for k in table if k.startswith(name + "(")]
    assert len(hits) == 1, (name, hits)
    r = table[hits[0]]
    print("CHEES_KERNEL", name, "vgpr", r["vgpr_count"], "sgpr", r["sgpr_count"], "lds", r["group_segment_fixed_size"])
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (hits[0], r)
