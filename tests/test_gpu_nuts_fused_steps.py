"""Fused NUTS on the built-in targets (pathfinder.jl_amd/csrc/nuts_fused_kernel.hip): EVERY recorded trip and EVERY decision against the
teacher-forced long-double checker of tests/nuts_reference.py, and every recorded value and gradient of the in-kernel target evaluation
against the long-double target of tests/hmc_fused_reference.py, with PFMI_NUTS_RECORD_PATH, max_depth 5, T = 3, K = 3.

Grid (hmc_fused_reference.GRID, 22 cases): d = 64 x history_length in {2, 4, 6, 8, 10, 16, 32} (all seven column paddings) x {Gaussian
rank-2, funnel}; d = 5, J = 10 (d < KPAD); d = 257, J = 6 on t_diag (rank padding 0), t_lowrank r = 12 (rank padding 16) and the funnel;
the funnel at d = 1600 and 1601, J = 6 (the two sides of pf_hmc_resident at KPAD 12); d = 320, J = 32 Gaussian (KPAD 64, streamed).
Chains as in tests/test_gpu_hmc_fused_steps.py (hmc_fused_reference.setup_chains).  The bounds are derived in the two references'
docstrings; borderline decisions (exempt) are capped at 2 % of a case's decisions.  Per case the run is ONE launch of the expected plan,
pfmi_nuts_stats is (1 + the most leaves a chain made, 0), and the chains' leaf counts differ: the workgroups leave the launch at different
trips.  Largest ratios seen: profiles/nuts_fused_parity.md."""
import json

import numpy as np
import pytest

import hmc_fused_reference as F
import hmc_reference as H
import margins as mg
import nuts_fused_reference as NF
import nuts_reference as N
from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not HAVE_LONGDOUBLE, reason=SKIP_REASON)]

_COV = {"cases": set(), "seen": set()}


def _run_case(pfmi_mod, eng, case):
    d, J, tn = case
    cid, kpad, md, T = NF.case_id(case), H.kpad_for(J), NF.GRID_DEPTH, NF.GRID_T
    tg, pts, x0, eps, seeds, jeff = F.setup_chains(pfmi_mod, eng, case, K=NF.GRID_K)
    plan = NF.plan_name(tg, d, kpad)
    before = eng.kernel_time(plan)[1]
    eng.nuts_fused_enqueue(pts, x0, seeds, eps, md, T, record_path=True)
    eng.nuts_wait()
    got, stats, path = eng.hmc_get(), eng.nuts_get_stats(), eng.nuts_path()
    leaves = np.sum(stats[1], axis=1)
    assert eng.nuts_stats() == (1 + int(np.max(leaves)), 0), (cid, eng.nuts_stats(), stats[1])
    assert eng.kernel_time(plan)[1] - before == 1, plan        # at most 94 trips: one launch of the expected instantiation
    assert len(set(leaves.tolist())) > 1, (cid, leaves)        # the chains left the launch at different trips
    borderline = decisions = 0
    for k in range(NF.GRID_K):
        p = int(pts[k])
        M = H.Metric.from_fit(eng.get_fit(p, int(jeff[p])))
        rec = N.gpu_recording(x0[:, k], path, got, stats, k)
        out = N.check(M, rec, int(seeds[k]), float(eps[k]), md, kpad, label=(cid, k))
        rl, rg = F.target_ratios(tg, rec["X"], rec["lp"], rec["g"])
        print("NUTS_FUSED_STEP", json.dumps({"case": cid, "k": k, "j_eff": int(jeff[p]), "depth": stats[0][k].tolist(), "leapfrog": stats[1][k].tolist(),
                                             "decisions": out["decisions"], "borderline": out["borderline"], "seen": sorted(out["seen"]),
                                             "lp": float("%.3g" % rl), "grad": float("%.3g" % rg),
                                             "margins": {q: float("%.3g" % m) for q, m in out["margins"].items()}}))
        mg.check("nuts_fused:" + cid, "nuts_fused_lp", [rl], 1.0)
        mg.check("nuts_fused:" + cid, "nuts_fused_grad", [rg], 1.0)
        for q, m in out["margins"].items():
            mg.check("nuts_fused:" + cid, "nuts_fused_" + q, [m], 1.0)
        # a chain's rows beyond its own trips were written by no one: their events keep t = -1
        ev = path[4]
        assert np.all(ev[1 + int(leaves[k]):, k]["t"] == -1), (cid, k)
        borderline += out["borderline"]
        decisions += out["decisions"]
        _COV["seen"] |= out["seen"]
    assert decisions > 0 and borderline <= (2 * decisions) // 100, (cid, borderline, decisions)
    _COV["cases"].add(cid)


@pytest.mark.parametrize("case", NF.GRID, ids=[NF.case_id(c) for c in NF.GRID])
def test_every_trip_decision_and_evaluation_matches_the_references(pfmi_mod, eng, case):
    _run_case(pfmi_mod, eng, case)


def test_grid_coverage(pfmi_mod, eng):
    """every nuts_fused plan of the grid was launched -- all seven paddings, both factor routes at KPAD 12, all four target shapes -- and
    the grid saw both directions, every stop reason, a divergence and both outcomes of the tree selection.  Cases that have not run in
    this session (a selection, a split over workers) are run here first"""
    for case in NF.GRID:
        if NF.case_id(case) not in _COV["cases"]:
            _run_case(pfmi_mod, eng, case)
    plans = NF.grid_plans(pfmi_mod)
    assert {int(p.split(":")[1]) for p in plans} == set(H.KPADS) and {p.split(":")[3] for p in plans} == {"f", "g0", "g8", "g16"}
    for plan in sorted(plans):
        assert eng.kernel_time(plan)[1] > 0, plan
    assert eng.kernel_time("nuts_fused:12:res:f")[1] > 0 and eng.kernel_time("nuts_fused:12:stream:f")[1] > 0
    assert _COV["seen"] >= NF.KINDS, _COV["seen"]
