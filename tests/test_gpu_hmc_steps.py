"""Static HMC step kernel (pathfinder.jl_amd/csrc/hmc_kernel.hip): EVERY recorded round and EVERY decision against the teacher-forced
long-double checker of tests/hmc_reference.py, through the example closure of examples/device_logp with PFMI_HMC_RECORD_PATH.

Grid (hmc_reference.GRID): d in {5, 64, 257, 1000} x history_length in {2, 6, 16, 32} (column padding 4, 12, 32, 64) x {Gaussian rank-2
target, funnel}, and history_length 4, 8, 10 (column padding 8, 16, 20) at d = 64 and 10 at d = 5 (d < KPAD = 20): all seven paddings
of hm_launch_step.  K = 3 chains whose metrics are the fits of a path's first point (j_eff = 0), of an early point with 0 < j_eff < J
and of the path's best fit; Lf = 3, T = 4; and one d = 20 000, J = 6 case (the factor rows streamed from HBM), T = 2.  Every chain starts
at the best fit's trace point; the three chains step by 0.4, 1 and 2.2 times d^(-1/4), so that small and large energy errors both occur.
The bounds are derived in hmc_reference's docstring; borderline decisions (exempt) are capped at 2 % of a case's transitions, i.e.
none at these sizes.  Largest ratios seen: profiles/hmc_step_parity.md."""
import json

import numpy as np
import pytest

import hmc_reference as H
import margins as mg
from helpers import demo_device_target, fit_seeds
from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON
from woodbury_reference import c_lane

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not HAVE_LONGDOUBLE, reason=SKIP_REASON)]

_COV = {"cases": set(), "accepted": 0, "rejected": 0}


def _run_case(pfmi_mod, eng, case):
    d, J, tn, T = case
    cid, kpad, Lf = H.case_id(case), H.kpad_for(J), H.GRID_LF
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
    x0 = np.asfortranarray(np.repeat(th[p_best][:, None], H.GRID_K, axis=1))
    eps, seeds = H.grid_eps(d), H.grid_seeds(d, J)
    plan = "hmc:%d:%s" % (kpad, "res" if H.resident(d, kpad) else "stream")
    before = eng.kernel_time(plan)[1]
    eng.hmc_enqueue(pts, x0, seeds, eps, Lf, T, record_path=True)
    eng.hmc_wait()
    assert eng.hmc_stats() == (1 + T * Lf, (1 + T * Lf) * H.GRID_K)
    assert eng.kernel_time(plan)[1] - before == 1 + T * Lf, plan      # exactly one launch per closure call, of the expected instantiation
    got, path = eng.hmc_get(), eng.hmc_path()
    borderline = 0
    z = np.random.default_rng(d + J).standard_normal(d)
    for k in range(H.GRID_K):
        p = int(pts[k])
        M = H.Metric.from_fit(eng.get_fit(p, int(jeff[p])))
        # the checker's operators are the library's: Metric.L / Metric.R against pfmi_woodbury_apply (PFMI_OP_UNWHITEN / PFMI_OP_RMUL) on this
        # fit, within the lane kernel's bound (woodbury_reference.c_lane: one fma per row, d + 3 KPAD + 16 roundings of the same absolute
        # sums), at every padding of the grid; the whole surface against long double: tests/test_gpu_woodbury.py
        for op, ref, scale in (("unwhiten", M.L(z), M.L_abs(np.abs(z))), ("rmul", M.R(z), M.R_abs(np.abs(z)))):
            dev = np.abs(eng.woodbury_apply(p, op, z) - ref) / (c_lane(d, kpad) * H.EPS * scale)
            mg.check("hmc:" + cid, "hmc_op_" + op, [dev.max()], 1.0)
        rec = H.gpu_recording(x0[:, k], path, got, k)
        out = H.check(M, rec, int(seeds[k]), float(eps[k]), Lf, kpad, label=(cid, k))
        print("HMC_STEP", json.dumps({"case": cid, "k": k, "j_eff": int(jeff[p]), "accepted": out["accepted"], "rejected": out["rejected"],
                                      "divergent": out["divergent"], "borderline": out["borderline"],
                                      "margins": {q: float("%.3g" % m) for q, m in out["margins"].items()}}))
        for q, m in out["margins"].items():
            mg.check("hmc:" + cid, "hmc_" + q, [m], 1.0)
        borderline += out["borderline"]
        _COV["accepted"] += out["accepted"]
        _COV["rejected"] += out["rejected"]
    assert borderline <= (2 * T * H.GRID_K) // 100, (cid, borderline)
    _COV["cases"].add(cid)


@pytest.mark.parametrize("case", H.GRID, ids=[H.case_id(c) for c in H.GRID])
def test_every_round_and_decision_matches_the_checker(pfmi_mod, eng, case):
    _run_case(pfmi_mod, eng, case)


def test_grid_coverage(pfmi_mod, eng):
    """every KPAD instantiation and both factor routes were launched, and the grid saw accepted and rejected transitions.  Cases that have
    not run in this session (a selection, a split over workers) are run here first: the assertions are always made"""
    for case in H.GRID:
        if H.case_id(case) not in _COV["cases"]:
            _run_case(pfmi_mod, eng, case)
    assert {H.kpad_for(c[1]) for c in H.GRID} == set(H.KPADS)
    for kpad in H.KPADS:
        assert sum(eng.kernel_time("hmc:%d:%s" % (kpad, r))[1] for r in ("res", "stream")) > 0, kpad
    assert eng.kernel_time("hmc:12:res")[1] > 0 and eng.kernel_time("hmc:12:stream")[1] > 0 and eng.kernel_time("hmc:64:stream")[1] > 0
    assert _COV["accepted"] > 0 and _COV["rejected"] > 0, _COV
