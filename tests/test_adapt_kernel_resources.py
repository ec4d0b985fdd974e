"""Build-time pin of the warm kernels (pf_hmc_warm_kernel, pf_nuts_warm_kernel: the step kernels' bodies with the step-size update of
csrc/adapt.h), read from the code objects of the library that was just built: all 14 instantiations of each exist exactly once, none uses
scratch or spills a vector register, each passes the LDS inequality of the plain kernels' tests (tests/test_hmc_kernel_resources.py,
tests/test_nuts_kernel_resources.py) and keeps its waves per SIMD, and the scalar registers moved into lanes of a vector register
(printed) stay within the 8 the project allows pf_nuts_step_kernel and within what the instantiation had before the passes were shared:
none for static HMC (the check itself: tests/chain_kernel_resources.py)."""
import pytest

import chain_kernel_resources as ckr
from chain_kernel_resources import KPADS

WARM = [(name, k, r) for name in ("pf_hmc_warm_kernel", "pf_nuts_warm_kernel") for k in KPADS for r in ("true", "false")]


@pytest.fixture(scope="module")
def table():
    return ckr.built_table()


@pytest.mark.parametrize("name,kpad,res", WARM, ids=["%s-%d-%s" % (n.split("_")[1], k, "res" if r == "true" else "stream") for n, k, r in WARM])
def test_warm_kernel_has_no_scratch_and_fits_lds(table, name, kpad, res):
    r = ckr.check_instantiation(table, name, kpad, res, "WARM_KERNEL")
    assert r["sgpr_spill_count"] <= (8 if "nuts" in name else 0), (name, kpad, res, r)


def test_no_other_warm_instantiation_exists(table):
    for name in ("pf_hmc_warm_kernel<", "pf_nuts_warm_kernel<"):
        assert len([k for k in table if k.startswith(name)]) == 2 * len(KPADS), name
