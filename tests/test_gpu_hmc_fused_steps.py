"""Fused static HMC on the built-in targets (pathfinder.jl_amd/csrc/hmc_fused_kernel.hip): EVERY recorded round and EVERY decision
against the teacher-forced long-double checker of tests/hmc_reference.py, and every recorded value and gradient of the in-kernel target
evaluation against the long-double target of tests/hmc_fused_reference.py, with PFMI_HMC_RECORD_PATH, T = 4, Lf = 3, K = 3.

Grid (hmc_fused_reference.GRID): d = 64 x history_length in {2, 4, 6, 8, 10, 16, 32} (all seven column paddings) x {Gaussian rank-2,
funnel}; d = 5, J = 10 (d < KPAD); d = 257, J = 6 on t_diag (rank padding 0), t_lowrank r = 12 (rank padding 16) and the funnel (one row
beyond a full sweep of the workgroup); the funnel at d = 1600 and 1601, J = 6 (the two sides of pf_hmc_resident at KPAD 12); d = 320,
J = 32 Gaussian (KPAD 64, streamed).  Chains as in tests/test_gpu_hmc_steps.py (hmc_fused_reference.setup_chains).  The bounds are
derived in the two references' docstrings; borderline decisions (exempt) are capped at 2 % of a case's transitions, i.e. none at these
sizes.  Largest ratios seen: profiles/hmc_fused_parity.md."""
import json

import numpy as np
import pytest

import hmc_fused_reference as F
import hmc_reference as H
import margins as mg
from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not HAVE_LONGDOUBLE, reason=SKIP_REASON)]

_COV = {"cases": set(), "accepted": 0, "rejected": 0}


def _run_case(pfmi_mod, eng, case):
    d, J, tn = case
    cid, kpad, Lf, T = F.case_id(case), H.kpad_for(J), F.GRID_LF, F.GRID_T
    tg, pts, x0, eps, seeds, jeff = F.setup_chains(pfmi_mod, eng, case)
    plan = F.plan_name(tg, d, kpad)
    before = eng.kernel_time(plan)[1]
    eng.hmc_fused_enqueue(pts, x0, seeds, eps, Lf, T, record_path=True)
    eng.hmc_wait()
    assert eng.hmc_stats() == (1 + T * Lf, 0)                  # evaluations, and no column ever went to a closure
    assert eng.kernel_time(plan)[1] - before == 1, plan        # 13 rounds: one launch of the expected instantiation
    got, path = eng.hmc_get(), eng.hmc_path()
    borderline = 0
    for k in range(F.GRID_K):
        p = int(pts[k])
        M = H.Metric.from_fit(eng.get_fit(p, int(jeff[p])))
        rec = H.gpu_recording(x0[:, k], path, got, k)
        out = H.check(M, rec, int(seeds[k]), float(eps[k]), Lf, kpad, label=(cid, k))
        rl, rg = F.target_ratios(tg, rec["X"], rec["lp"], rec["g"])
        print("HMC_FUSED_STEP", json.dumps({"case": cid, "k": k, "j_eff": int(jeff[p]), "accepted": out["accepted"], "rejected": out["rejected"],
                                            "divergent": out["divergent"], "borderline": out["borderline"], "lp": float("%.3g" % rl),
                                            "grad": float("%.3g" % rg), "margins": {q: float("%.3g" % m) for q, m in out["margins"].items()}}))
        mg.check("hmc_fused:" + cid, "hmc_fused_lp", [rl], 1.0)
        mg.check("hmc_fused:" + cid, "hmc_fused_grad", [rg], 1.0)
        for q, m in out["margins"].items():
            mg.check("hmc_fused:" + cid, "hmc_fused_" + q, [m], 1.0)
        borderline += out["borderline"]
        _COV["accepted"] += out["accepted"]
        _COV["rejected"] += out["rejected"]
    assert borderline <= (2 * T * F.GRID_K) // 100, (cid, borderline)
    _COV["cases"].add(cid)


@pytest.mark.parametrize("case", F.GRID, ids=[F.case_id(c) for c in F.GRID])
def test_every_round_decision_and_evaluation_matches_the_references(pfmi_mod, eng, case):
    _run_case(pfmi_mod, eng, case)


def test_grid_coverage(pfmi_mod, eng):
    """every hmc_fused plan of the grid was launched -- all seven paddings, both factor routes, all four target shapes -- and the grid saw
    accepted and rejected transitions.  Cases that have not run in this session (a selection, a split over workers) are run here first"""
    for case in F.GRID:
        if F.case_id(case) not in _COV["cases"]:
            _run_case(pfmi_mod, eng, case)
    plans = F.grid_plans(pfmi_mod)
    assert {int(p.split(":")[1]) for p in plans} == set(H.KPADS) and {p.split(":")[3] for p in plans} == {"f", "g0", "g8", "g16"}
    for plan in sorted(plans):
        assert eng.kernel_time(plan)[1] > 0, plan
    assert eng.kernel_time("hmc_fused:12:res:f")[1] > 0 and eng.kernel_time("hmc_fused:12:stream:f")[1] > 0
    assert _COV["accepted"] > 0 and _COV["rejected"] > 0, _COV
