"""Build-time pin of the warm kernels (pf_hmc_warm_kernel, pf_nuts_warm_kernel: the step kernels' bodies with the step-size update of
csrc/adapt.h), read from the code objects of the library that was just built: all 14 instantiations of each exist exactly once, none uses
scratch or spills a vector register, each passes the LDS inequality of the plain kernels' tests (tests/test_hmc_kernel_resources.py,
tests/test_nuts_kernel_resources.py), and the scalar registers moved into lanes of a vector register (printed) stay within the 8 the
project allows pf_nuts_step_kernel."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pathfinder.jl_amd", "tools"))

KPADS = (4, 8, 12, 16, 20, 32, 64)
LDS_LIMIT = 160 * 1024
LDS_RES = 150 * 1024
WARM = [(name, k, r) for name in ("pf_hmc_warm_kernel", "pf_nuts_warm_kernel") for k in KPADS for r in ("true", "false")]


@pytest.fixture(scope="module")
def table():
    import kernel_resources as kr
    import pfmi
    pfmi.build()
    return kr.kernel_resources()


@pytest.mark.parametrize("name,kpad,res", WARM, ids=["%s-%d-%s" % (n.split("_")[1], k, "res" if r == "true" else "stream") for n, k, r in WARM])
def test_warm_kernel_has_no_scratch_and_fits_lds(table, name, kpad, res):
    prefix = f"{name}<{kpad}, {res}>("
    hits = [k for k in table if k.startswith(prefix)]
    assert len(hits) == 1, (prefix, hits)
    r = table[hits[0]]
    print("WARM_KERNEL", hits[0].split("(")[0], "vgpr", r["vgpr_count"], "sgpr", r["sgpr_count"], "sgpr to lanes", r["sgpr_spill_count"], "lds",
          r["group_segment_fixed_size"])
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] <= 8, (hits[0], r)
    static = r["group_segment_fixed_size"]
    nred = max(kpad + 4, 24) if "nuts" in name else kpad + 4
    assert static >= 8 * (2 * 4 * nred + 3 * kpad), (hits[0], r)
    assert static + (LDS_RES if res == "true" else 0) <= LDS_LIMIT, (hits[0], r)
    assert r["vgpr_count"] <= 512, (hits[0], r)


def test_no_other_warm_instantiation_exists(table):
    for name in ("pf_hmc_warm_kernel<", "pf_nuts_warm_kernel<"):
        assert len([k for k in table if k.startswith(name)]) == 2 * len(KPADS), name
