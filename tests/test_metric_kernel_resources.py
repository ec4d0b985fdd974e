"""Build-time pin of the metric kernels (pf_hmc_metric_kernel, pf_nuts_metric_kernel: the step bodies of csrc/hmc_kernel.hip and
csrc/nuts_kernel.hip in their third mode -- a per-coordinate scale, the whiten pass and the Welford update of csrc/hmc_rows.h), read from the
code objects of the library that was just built: all 14 instantiations of each exist exactly once, none uses scratch or spills a vector
register, and the static LDS of each leaves the HM_LDS_RES bytes of staged factor rows inside the 160 KB of a compute unit.  Scalar
registers moved into lanes of a vector register are printed, not capped: they cost no memory traffic.  (That the step and warm kernels did
not move is what tests/test_hmc_kernel_resources.py, test_nuts_kernel_resources.py and test_adapt_kernel_resources.py pin.)"""
import pytest

import chain_kernel_resources as ckr
from chain_kernel_resources import KPADS, LDS_LIMIT, LDS_RES

METRIC = [(name, k, r) for name in ("pf_hmc_metric_kernel", "pf_nuts_metric_kernel") for k in KPADS for r in ("true", "false")]


@pytest.fixture(scope="module")
def table():
    return ckr.built_table()


@pytest.mark.parametrize("name,kpad,res", METRIC, ids=["%s-%d-%s" % (n.split("_")[1], k, "res" if r == "true" else "stream") for n, k, r in METRIC])
def test_metric_kernel_has_no_scratch_and_fits_lds(table, name, kpad, res):
    prefix = f"{name}<{kpad}, {res}>("
    hits = [k for k in table if k.startswith(prefix)]
    assert len(hits) == 1, (prefix, hits)
    r = table[hits[0]]
    print("METRIC_KERNEL", hits[0].split("(")[0], "vgpr", r["vgpr_count"], "sgpr", r["sgpr_count"], "sgpr to lanes", r["sgpr_spill_count"], "lds",
          r["group_segment_fixed_size"])
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (hits[0], r)
    static = r["group_segment_fixed_size"]
    nred = max(kpad + 4, 24) if "nuts" in name else kpad + 4
    assert static >= 8 * (2 * 4 * nred + 3 * kpad), (hits[0], r)                 # the ping-pong reduction buffers, sHead, sZ, sTv
    assert static + (LDS_RES if res == "true" else 0) <= LDS_LIMIT, (hits[0], r)
    assert r["vgpr_count"] <= 512, (hits[0], r)


def test_no_other_metric_instantiation_exists(table):
    for name in ("pf_hmc_metric_kernel<", "pf_nuts_metric_kernel<"):
        assert len([k for k in table if k.startswith(name)]) == 2 * len(KPADS), name
