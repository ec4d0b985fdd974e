"""Device L-BFGS (lbfgs_kernels.hip, lbfgs_closure_kernel.hip): EVERY recorded step against the extended-precision replay of
tests/lbfgs_step_reference.py -- the direction from the kernel's own x_l and its own ring (rebuilt bit for bit from the trace), the
step length against the replayed strong-Wolfe search, the curvature rule, the stop rules -- at every instantiation pf_launch_lbfgs
dispatches to, with the ring full and wrapped, over ragged reduction batches, and through the pair-rejected second pass
(PFMI_LBFGS_REJECT_EVERY).  Errors do not accumulate along a teacher-forced trace: step 60 is held as tightly as step 1, which the
first-iterates comparisons of test_gpu_fit.py / test_gpu_closure_lbfgs.py cannot do.

The grid (shapes, starts, iteration limits) lives in lbfgs_step_reference.GRID / CLOSURE_GRID; tests/test_lbfgs_step_cpu.py runs the
same cases through both CPU drivers, proves that the grid reaches every instantiation and that the checker catches a wrong Gram entry,
gamma, ring slot or initial step.  Largest ratios seen: profiles/lbfgs_step_parity.md."""
import json

import numpy as np
import pytest

from helpers import demo_device_target
import lbfgs_step_reference as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.HAVE_LONGDOUBLE, reason=R.SKIP_REASON)]

_KEYS = ("steps", "max_h", "wrapped", "turns", "rejected", "restarts", "exempt", "borderline", "max_ratio_a", "max_tau_factor", "max_ratio_b", "max_dev64", "stop")


def _run_case(pfmi_mod, eng, monkeypatch, case, closure):
    cid, tn, d, J, maxit, rej, sc = case
    assert maxit <= 120
    tg = R.grid_target(pfmi_mod, tn, d)
    x0 = R.grid_x0(pfmi_mod, d, sc)
    dev_tg = demo_device_target(tg, grad=True) if closure else tg
    e = eng
    if rej:                                                  # the hook is read from the environment: a fresh engine, as the existing
        monkeypatch.setenv("PFMI_LBFGS_REJECT_EVERY", str(rej))      # rejected-pair test does
        e = pfmi_mod.Engine(0)
    try:
        e.set_target(dev_tg)
        npts = e.optimize_batch(x0, J, maxit, R.G_TOL)
        traces = [e.get_trace(k) for k in range(R.GRID_K)]
    finally:
        if rej:
            e.close()
            monkeypatch.delenv("PFMI_LBFGS_REJECT_EVERY")
    for k, (th, lp, gr) in enumerate(traces):
        assert th.shape == (npts[k], d) and np.array_equal(th[0], x0[k]) and 2 <= npts[k] <= maxit + 1
        recs, s = R.check_trace(th, lp, gr, J, maxit, R.G_TOL, fg=tg.logp_and_grad, reject_every=rej)
        print("LBFGS_STEP", json.dumps({"case": cid, "k": k, **{q: s[q] for q in _KEYS}, "first_failure": s["first_failure"]}))
        R.assert_trace(cid, recs, s, J, impl="gpu")
        assert R.coverage_ok(s, J), (cid, k, "coverage", s["wrapped"], s["turns"], s["steps"])
        assert s["max_h"] == J
        if rej:
            assert s["rejected"] >= s["steps"] // rej


@pytest.mark.parametrize("case", R.GRID, ids=[c[0] for c in R.GRID])
def test_device_lbfgs_every_step_matches_the_replay(pfmi_mod, eng, monkeypatch, case):
    """pf_lbfgs_kernel<EPT, NT, RPAD, ring in LDS | global>: K = 2 paths per case"""
    _run_case(pfmi_mod, eng, monkeypatch, case, closure=False)


@pytest.mark.parametrize("case", R.CLOSURE_GRID, ids=[c[0] for c in R.CLOSURE_GRID])
def test_closure_lbfgs_every_step_matches_the_replay(pfmi_mod, eng, monkeypatch, case):
    """pf_lbc_step_kernel on the example closure of examples/device_logp: J = 6, 24, 32 (batches of 4 slots, the last one full or
    ragged), d = 20 000 (beyond the built-in kernel), one case through the pair-rejected branch; fg is the target's host function"""
    _run_case(pfmi_mod, eng, monkeypatch, case, closure=True)
