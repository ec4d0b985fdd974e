"""Build-time pin of the fused metric kernels (csrc/hmc_fused_metric_kernel.hip, csrc/nuts_fused_metric_kernel.hip), read from the code
objects of the library that was just built (pathfinder.jl_amd/tools/kernel_resources.py, through tests/chain_kernel_resources.py): every
instantiation the launchers can take -- column padding 4 .. 64 x factor rows staged in LDS or streamed x {funnel, Gaussian family with
rank padding 0, 8, 16}: 56 per sampler -- compiles for gfx950 without scratch and without a spilled vector register, holds the LDS of its
reductions (static HMC: the wider of KPAD + 4 and RPAD + 4 values; NUTS: also the 24 dot products of a leaf's decisions), the three
KPAD-long vectors and G's copy, and leaves the HM_LDS_RES bytes of staged factor rows inside the 160 KB of a compute unit.  Scalar
registers moved into lanes of a vector register are printed, not capped, as for the fused kernels.  Also: the C ABI and the ctypes
binding carry the two entry points, and the sources keep the rules the kernels' headers state (one loop, no qualifier on the scale)."""
import os
import re

import pytest

import chain_kernel_resources as ckr
from chain_kernel_resources import KPADS, LDS_LIMIT, LDS_RES

TARGETS = (-1, 0, 8, 16)                                        # HM_TG_FUNNEL, then the Gaussian family's rank paddings
SAMPLERS = ("hmc", "nuts")
LAUNCHED = [(s, k, r, t) for s in SAMPLERS for k in KPADS for r in ("true", "false") for t in TARGETS]
CSRC = os.path.join(ckr.ROOT, "pathfinder.jl_amd", "csrc")


@pytest.fixture(scope="module")
def table():
    return ckr.built_table()


def nred_of(sampler, kpad, tg):
    """the widest reduction of the kernel, as tests/test_hmc_fused_kernel_resources.py and test_nuts_fused_kernel_resources.py compute it"""
    rpad = tg if tg > 0 else 0
    return max(kpad + 4, rpad + 4 if rpad else 4) if sampler == "hmc" else max(kpad + 4, 24, rpad + 4)


@pytest.mark.parametrize("sampler,kpad,res,tg", LAUNCHED)
def test_fused_metric_kernel_has_no_scratch_no_spills_and_fits_lds(table, sampler, kpad, res, tg):
    prefix = f"pf_{sampler}_fused_metric_kernel<{kpad}, {res}, {tg}>("
    hits = [k for k in table if k.startswith(prefix)]
    assert len(hits) == 1, (prefix, hits)
    r = table[hits[0]]
    print("FUSED_METRIC_KERNEL", hits[0].split("(")[0], "vgpr", r["vgpr_count"], "agpr", r["agpr_count"], "sgpr", r["sgpr_count"], "sgpr to lanes",
          r["sgpr_spill_count"], "lds", r["group_segment_fixed_size"])
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (hits[0], r)
    G = tg * tg if tg > 0 else 0
    static = r["group_segment_fixed_size"]
    assert static >= 8 * (2 * 4 * nred_of(sampler, kpad, tg) + 3 * kpad + G), (hits[0], r)
    assert static + (LDS_RES if res == "true" else 0) <= LDS_LIMIT, (hits[0], r)
    assert r["vgpr_count"] <= 512, (hits[0], r)                 # 256 threads: one wave per SIMD, all 512 registers (VGPR + AGPR)


def test_every_instantiation_is_built_once_and_the_fused_kernels_keep_their_count(table):
    for sampler in SAMPLERS:
        assert len([k for k in table if k.startswith(f"pf_{sampler}_fused_metric_kernel<")]) == 56, sampler
        assert len([k for k in table if k.startswith(f"pf_{sampler}_fused_kernel<")]) == 56, sampler


def test_the_abi_and_the_binding_carry_both_entry_points():
    import ctypes

    import pfmi
    from pfmi import _lib
    lib = ctypes.CDLL(pfmi.build())
    header = open(os.path.join(ckr.ROOT, "include", "pfmi.h")).read()
    for name in ("pfmi_hmc_fused_metric_enqueue", "pfmi_nuts_fused_metric_enqueue"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS and re.search(r"\bint32_t %s\(" % name, header), name
        assert _lib.ARGTYPES[name] == _lib.ARGTYPES[name.replace("_metric", "")], name               # the argument list of the fused enqueue
    for method in ("hmc_fused_metric_enqueue", "nuts_fused_metric_enqueue"):
        assert callable(getattr(pfmi.Engine, method))


def test_one_loop_and_no_qualifier_on_the_scale():
    """the metric translation units define no loop of their own (they expand the fused sources' loop), and nothing on the way from
    HmMetric::scale to its uses promises the compiler that the scale is not written"""
    for sampler, loop in (("hmc", "HM_FUSED_LOOP("), ("nuts", "NT_FUSED_LOOP(")):
        text = open(os.path.join(CSRC, f"{sampler}_fused_metric_kernel.hip")).read()
        code = "\n".join(line.split("//")[0] for line in text.splitlines())
        assert f'#include "{sampler}_fused_kernel.hip"' in code and loop in code
        assert "for (" not in code and "while (" not in code and "_round<" not in code, sampler
        for word in ("__restrict__", "__builtin_nontemporal", "__ldg", "__syncthreads", "__hip_atomic", "atomic"):
            assert word not in code, (sampler, word)
    rows = open(os.path.join(CSRC, "hmc_rows.h")).read()
    assert re.search(r"struct HmMetric \{\s*double \*scale;", rows)                                   # a plain pointer to doubles
    for name in ("hmc_rows.h", "hmc_kernel.hip", "nuts_kernel.hip", "hmc_fused_kernel.hip", "nuts_fused_kernel.hip"):
        text = open(os.path.join(CSRC, name)).read()
        for line in text.splitlines():
            code = line.split("//")[0]
            if "scale" in code:
                assert "__restrict__" not in code and "nontemporal" not in code and "__ldg" not in code, (name, line)
