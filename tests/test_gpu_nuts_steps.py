"""NUTS step kernel (pathfinder.jl_amd/csrc/nuts_kernel.hip): EVERY recorded round and EVERY decision against the teacher-forced long-double
checker of tests/nuts_reference.py, through the example closure of examples/device_logp with PFMI_NUTS_RECORD_PATH.

Grid (nuts_reference.GRID): d in {5, 64, 257, 1000} x history_length in {2, 6, 16, 32} (column padding 4, 12, 32, 64) x {Gaussian rank-2
target, funnel}, and history_length 4, 8, 10 (column padding 8, 16, 20) at d = 64 and 10 at d = 5 (d < KPAD = 20): all seven paddings
of hm_launch_step.  K = 3 chains on the fits tests/test_gpu_hmc_steps.py picks (a path's first point, an early point with
0 < j_eff < J, the best fit), stepping by 0.4, 1 and 2.2 times d^(-1/4); max_depth 5, T = 3; and one d = 20 000, J = 6 case (the factor rows streamed from
HBM), max_depth 3, T = 1.  The bounds are derived in nuts_reference's docstring; borderline decisions (exempt) are capped at 2 % of a
case's decisions, i.e. none at these sizes.  Largest ratios seen: profiles/nuts_step_parity.md."""
import json

import numpy as np
import pytest

import hmc_reference as H
import margins as mg
import nuts_reference as N
from helpers import demo_device_target, fit_seeds
from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not HAVE_LONGDOUBLE, reason=SKIP_REASON)]

_COV = {"cases": set(), "seen": set()}


def _run_case(pfmi_mod, eng, case):
    d, J, tn, md, T = case
    cid, kpad = N.case_id(case), H.kpad_for(J)
    tg = H.grid_target(pfmi_mod, tn, d)
    eng.set_target(demo_device_target(tg, grad=True))
    npts = eng.optimize_batch(H.grid_path_x0(pfmi_mod, tn, d), J, 40, 1e-8)
    eng.fit_batch(J)
    status, jeff, _, _ = eng.fit_status()
    P = int(npts[0])
    _, _, best = eng.elbo_batch(32, fit_seeds(P, 5))
    p_best = int(best[0])
    early = [p for p in range(1, P) if status[p] == 0 and 0 < jeff[p] < J]
    assert status[0] == 0 and jeff[0] == 0 and early and status[p_best] == 0, (cid, status[:4], jeff[:4], p_best)
    pts = np.array([0, early[0], p_best], dtype=np.int64)
    th, _, _ = eng.get_trace(0)
    x0 = np.asfortranarray(np.repeat(th[p_best][:, None], N.GRID_K, axis=1))
    eps, seeds = H.grid_eps(d), H.grid_seeds(d, J)
    plan = "nuts:%d:%s" % (kpad, "res" if H.resident(d, kpad) else "stream")
    before = eng.kernel_time(plan)[1]
    eng.nuts_enqueue(pts, x0, seeds, eps, md, T, record_path=True)
    eng.nuts_wait()
    got, stats, path = eng.hmc_get(), eng.nuts_get_stats(), eng.nuts_path()
    rounds, columns = eng.nuts_stats()
    assert rounds == 1 + int(np.max(np.sum(stats[1], axis=1))) and rounds <= 1 + T * (2 ** md - 1), (cid, rounds, stats[1])
    # exactly one launch per closure call, of the expected instantiation; the rounds issued ahead of the last progress word are a window's
    assert eng.kernel_time(plan)[1] - before == columns // N.GRID_K and rounds <= columns // N.GRID_K <= rounds + 4, (plan, rounds, columns)
    borderline = decisions = 0
    for k in range(N.GRID_K):
        p = int(pts[k])
        M = H.Metric.from_fit(eng.get_fit(p, int(jeff[p])))
        rec = N.gpu_recording(x0[:, k], path, got, stats, k)
        out = N.check(M, rec, int(seeds[k]), float(eps[k]), md, kpad, label=(cid, k))
        print("NUTS_STEP", json.dumps({"case": cid, "k": k, "j_eff": int(jeff[p]), "depth": stats[0][k].tolist(), "leapfrog": stats[1][k].tolist(),
                                       "decisions": out["decisions"], "borderline": out["borderline"], "seen": sorted(out["seen"]),
                                       "margins": {q: float("%.3g" % m) for q, m in out["margins"].items()}}))
        for q, m in out["margins"].items():
            mg.check("nuts:" + cid, "nuts_" + q, [m], 1.0)
        borderline += out["borderline"]
        decisions += out["decisions"]
        _COV["seen"] |= out["seen"]
    assert decisions > 0 and borderline <= (2 * decisions) // 100, (cid, borderline, decisions)
    _COV["cases"].add(cid)


@pytest.mark.parametrize("case", N.GRID, ids=[N.case_id(c) for c in N.GRID])
def test_every_round_and_decision_matches_the_checker(pfmi_mod, eng, case):
    _run_case(pfmi_mod, eng, case)


def test_grid_coverage(pfmi_mod, eng):
    """every KPAD instantiation and both factor routes were launched, and the grid saw both directions, every stop reason, a divergence and
    both outcomes of the top-level selection.  Cases that have not run in this session (a selection, a split over workers) are run here
    first: the assertions are always made"""
    for case in N.GRID:
        if N.case_id(case) not in _COV["cases"]:
            _run_case(pfmi_mod, eng, case)
    assert {H.kpad_for(c[1]) for c in N.GRID} == set(H.KPADS)
    for kpad in H.KPADS:
        assert sum(eng.kernel_time("nuts:%d:%s" % (kpad, r))[1] for r in ("res", "stream")) > 0, kpad
    assert eng.kernel_time("nuts:12:res")[1] > 0 and eng.kernel_time("nuts:12:stream")[1] > 0 and eng.kernel_time("nuts:64:stream")[1] > 0
    assert _COV["seen"] >= {"dir+", "dir-", "subtree_turn", "tree_turn", "max_depth", "divergent", "candidate_replaced", "candidate_kept"}, _COV["seen"]
