"""Pins tests/nuts_fused_reference.py on the CPU: nuts_reference's mirror and checker, driven by the built-in targets' host logp_and_grad,
on the grid of tests/test_gpu_nuts_fused_steps.py (synthetic factors of the fits' shapes, as tests/test_nuts_reference_cpu.py builds them)
with ZERO borderline decisions -- so the 2 % cap of the GPU test is met by the reference alone -- reaching all eight kinds of event and
every plan name of the fused kernel; the chains' leaf counts differ, so a launch sees chains leave at different trips.  CPU only."""
import numpy as np
import pytest

from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON

if not HAVE_LONGDOUBLE:
    pytest.skip(SKIP_REASON, allow_module_level=True)

import hmc_fused_reference as F                                # noqa: E402
import hmc_reference as H                                      # noqa: E402
import margins as mg                                           # noqa: E402
import nuts_fused_reference as NF                              # noqa: E402
import nuts_reference as N                                     # noqa: E402

_SEEN = {"kinds": set(), "cases": set(), "decisions": 0, "leaves": []}


@pytest.fixture(scope="module")
def pfmi_cpu():
    import pfmi
    return pfmi


def _grid_chains(pfmi, case):
    """the case's three chains on the mirror: factors with j_eff = 0, 0 < j_eff < J and j_eff = J"""
    d, J, tn = case
    tg = F.grid_target(pfmi, tn, d)
    rng = np.random.default_rng(7 * d + J)
    x0 = (np.zeros(d) if tn == "funnel" else tg.mean) + 0.1 * rng.standard_normal(d)
    eps, seeds = H.grid_eps(d), H.grid_seeds(d, J)
    for k, j in enumerate((0, max(1, J // 2), J)):
        M = H.random_metric(d, j, rng)
        M.s *= 0.5 if tn == "funnel" else 1.0
        yield k, tg, M, x0, int(seeds[k]), float(eps[k])


def _run_case(pfmi, case):
    d, J, tn = case
    kpad = H.kpad_for(J)
    leaves = []
    for k, tg, M, x0, seed, eps in _grid_chains(pfmi, case):
        rec = N.mirror(M, tg.logp_and_grad, x0, seed, eps, NF.GRID_DEPTH, NF.GRID_T)
        out = N.check(M, rec, seed, eps, NF.GRID_DEPTH, kpad, label=(NF.case_id(case), k))
        assert out["borderline"] == 0 and out["decisions"] > 0, (case, k, out)
        for q, m in out["margins"].items():
            mg.record("cpu:" + NF.case_id(case), "nuts_fused_" + q, [m], 1.0)
        # the mirror's evaluations are the host target's (NumPy's sums, not the kernel's reduction map): hmc_fused_reference's bound with
        # C = d + 3 RPAD + 16 (tests/test_hmc_fused_reference_cpu.py)
        rl, rg = F.target_ratios(tg, rec["X"], rec["lp"], rec["g"])
        host = F.c_target(d, F.rpad_of(tg)) / (d + 3 * F.rpad_of(tg) + 16.0)
        assert rl * host <= 1.0 and rg * host <= 1.0, (case, k, rl, rg)
        _SEEN["kinds"] |= out["seen"]
        _SEEN["decisions"] += out["decisions"]
        leaves.append(int(np.sum(rec["n_leapfrog"])))
    assert len(set(leaves)) > 1, (case, leaves)               # the chains leave their launch at different trips
    _SEEN["leaves"] += leaves
    _SEEN["cases"].add(NF.case_id(case))


@pytest.mark.parametrize("case", NF.GRID, ids=[NF.case_id(c) for c in NF.GRID])
def test_mirror_on_the_built_in_targets_passes_the_checker_without_borderline_decisions(pfmi_cpu, case):
    _run_case(pfmi_cpu, case)


def test_grid_reaches_every_kind_of_event_and_every_plan(pfmi_cpu):
    for case in NF.GRID:
        if NF.case_id(case) not in _SEEN["cases"]:
            _run_case(pfmi_cpu, case)
    print("NUTS_FUSED_GRID", sorted(_SEEN["kinds"]), _SEEN["decisions"], min(_SEEN["leaves"]), max(_SEEN["leaves"]))
    assert _SEEN["kinds"] >= NF.KINDS, _SEEN["kinds"]
    assert len(NF.GRID) == 22 and {H.kpad_for(J) for _, J, _ in NF.GRID} == set(H.KPADS)
    plans = NF.grid_plans(pfmi_cpu)
    assert {p.rsplit(":", 1)[1] for p in plans} == {"f", "g0", "g8", "g16"}
    assert {"nuts_fused:12:res:f", "nuts_fused:12:stream:f", "nuts_fused:64:stream:g8", "nuts_fused:20:res:g8"} <= plans
    assert NF.launches_bound(94, 7) == (14, 18) and NF.launches_bound(94, 1024) == (1, 5)
