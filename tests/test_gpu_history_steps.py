"""The history walk -- pf_history_kernel<EPT, NT>, pf_history_lean_kernel<EPT> and pf_history_mem_kernel -- against the long-double
replay of tests/history_reference.py: every step of every path, teacher-forced, at every one of the 17 instantiations and at the
lowest and the highest d of each.  Every case asserts the single plan it ran by the delta of the host-side launch counters
(pfmi_kernel_time "hist:reg:..", "hist:lean:..", "hist:mem", include/pfmi.h).  The cases are history_reference.GRID;
tests/test_history_reference_cpu.py proves on the CPU that they reach every plan, that two correct double walks stay inside the same
bound and that seven faulty walks do not.

What is asserted per path (the bound and its derivation are in the docstring of tests/history_reference.py):
  alpha of the first point is exactly 1, its j_eff is 0; j_eff and n_rejected are array-equal with the replay's
  after a rejected step alpha is bit-equal to the previous point's
  after an accepted step EVERY coordinate is within the counted bound of the replay from the device's own alpha of the previous point
  nocedal_wright: all coordinates of a point are bit-equal to each other
  the S block of pfmi_get_fit's B is bit-equal to the differences of the replayed ring's sources (a subtraction is exactly rounded)
The last section resumes the walk across launches (HistSeg, the streaming pipeline) on the families the stream tests never reached."""
import json

import numpy as np
import pytest

from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON

if not HAVE_LONGDOUBLE:
    pytest.skip(SKIP_REASON, allow_module_level=True)

import history_reference as hr                                 # noqa: E402
import margins as mg                                           # noqa: E402
from test_gpu_stream import _compare, _packed, _streamed        # noqa: E402

pytestmark = pytest.mark.gpu

_SEEN = set()
_DONE = set()
HOOK = "PFMI_HISTORY_KERNEL"
IDS = [hr.case_id(c) for c in hr.GRID]


def _counts(eng):
    return {nm: eng.kernel_time(nm)[1] for nm in hr.ALL_PLANS}


def _walk_asserting(eng, monkeypatch, c, eps, expect):
    """fit_batch(J, eps, hinit) under the case's PFMI_HISTORY_KERNEL and the assertion that exactly one walk was launched, of plan `expect`"""
    before = _counts(eng)
    if c.force:
        monkeypatch.setenv(HOOK, c.force)
    else:
        monkeypatch.delenv(HOOK, raising=False)
    try:
        eng.fit_batch(hr.J, eps, c.hinit)
    finally:
        monkeypatch.delenv(HOOK, raising=False)
    after = _counts(eng)
    delta = {k: after[k] - before[k] for k in hr.ALL_PLANS if after[k] != before[k]}
    assert delta == {expect: 1}, (delta, expect)
    assert eng.kernel_time("hist:")[1] == 0 and eng.kernel_time("hist:reg:3,64")[1] == 0      # an unknown plan name counts nothing
    _SEEN.add(expect)


def _run_case(pfmi, eng, monkeypatch, i):
    if i in _DONE:
        return
    c = hr.GRID[i]
    plan = hr.case_plan(c)
    th, gr = hr.case_traces(c)
    eps, reps = hr.case_replays(c, th, gr)
    eng.set_target(pfmi.t_iso(c.d))
    eng.set_traces(th, gr)
    _walk_asserting(eng, monkeypatch, c, eps, plan)
    status, jeff, logdet, nrej = eng.fit_status()
    assert eng.P == sum(hr.LENGTHS)
    worst, xc, failures, acc, rej = 0.0, np.inf, [], 0, 0
    for k, rep in enumerate(reps):
        p0 = int(eng.offsets[k])
        fits = [eng.get_fit(p0 + l, int(jeff[p0 + l])) for l in range(rep.n)]
        alpha = np.stack([f["alpha"] for f in fits])
        r, fails = hr.check_path(rep, plan, alpha, jeff[p0:p0 + rep.n], nrej[k],
                                 lambda l: fits[l]["B"][:, fits[l]["j"]:2 * fits[l]["j"]])
        worst, xc = max(worst, r["ratio"]), min(xc, r["x_cond"])
        acc, rej = acc + r["accepted"], rej + r["rejected"]
        failures += [(k,) + f for f in fails]
    print(json.dumps({"case": IDS[i], "plan": plan, "points": int(eng.P), "accepted": acc, "rejected": rej,
                      "largest_error_over_bound": float(f"{worst:.3g}"), "x_cond": float(f"{xc:.3g}")}))
    assert not failures, (IDS[i], plan, failures[:6])
    mg.check(plan, "hist_alpha_bound@gpu_vs_ld", worst, 1.0, ctx=IDS[i],
             why="error / counted bound (tests/history_reference.py), largest over every coordinate of every accepted step, one entry per case")
    _DONE.add(i)


# ---- 1. every plan, every step ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(hr.GRID)), ids=IDS)
def test_walk_every_plan_matches_the_replay(pfmi_mod, eng, monkeypatch, i):
    """all 17 instances at the lowest and the highest d of their range, six paths of 1, 2 and 12 .. 15 points (every remainder of the
    unrolled loop, a ring of J = 3 that wraps several times), a third of the steps rejected mid-trace; d = 1 with every step accepted and
    with every step rejected; per family the default eps, nocedal_wright and a planted NaN: the plan counter named by
    history_reference.plan_for rises by one, no other walk counter moves, and every path passes check_path"""
    _run_case(pfmi_mod, eng, monkeypatch, i)


# ---- 2. coverage ---------------------------------------------------------------------------------------------------------------------------
def test_union_of_plans_run_equals_reachable(pfmi_mod, eng, monkeypatch):
    """every plan of the CPU mirror was launched by this module (the grid cases run here if they have not run yet), and nothing else"""
    for i in range(len(hr.GRID)):
        _run_case(pfmi_mod, eng, monkeypatch, i)
    assert _SEEN == set(hr.REACHABLE), (sorted(set(hr.REACHABLE) - _SEEN), sorted(_SEEN - set(hr.REACHABLE)))
    assert len(_SEEN) == 17


# ---- 3. resume: the walk continued across launches on the families that have never resumed -----------------------------------------------------
RESUME = [(4100, None, "hist:lean:6"), (8200, None, "hist:lean:10"), (10300, None, "hist:reg:12,1024"), (300, b"mem", "hist:mem")]


@pytest.mark.parametrize("d,force,plan", RESUME, ids=[p for _, _, p in RESUME])
def test_resumed_walk_is_bit_identical_to_the_packed_route(pfmi_mod, d, force, plan):
    """the streaming pipeline cuts the walk into segments (HistSeg): the lean kernels restore 1 / alpha into LDS (EPT >= 9 re-reads the
    previous row), the 12-coordinate register kernel its carried reciprocal, the memory-resident kernel only its count.  Streamed and
    packed agree bit for bit, and the plan was launched at least twice by the streaming engine: something did resume."""
    assert hr.plan_for(d, "mem" if force else None) == plan
    L = pfmi_mod.lib()
    tg = pfmi_mod.t_diag(d, seed=1)
    K, J, maxiters, N = 3, 5, 40, 16
    cap = maxiters + 1
    x0 = pfmi_mod.HostRNG(31).rand(K * d).reshape(K, d) * 4 - 2
    sd = pfmi_mod.hostrng.rand_u64(77, np.arange(K * cap, dtype=np.uint64), 9)
    hooks = [(b"PFMI_STREAM_POLICY", b"1"), (b"PFMI_STREAM_PUB", b"4")] + ([(b"PFMI_HISTORY_KERNEL", force)] if force else [])
    for key, val in hooks:
        assert L.pfmi_debug_set(key, val) == 0
    try:
        a = _packed(pfmi_mod, tg, x0, J, maxiters, N, sd, N, 50)
        s = _streamed(pfmi_mod, tg, x0, J, maxiters, N, sd, N, 50, count=(plan,))[0]
    finally:
        for key, _ in hooks:
            assert L.pfmi_debug_set(key, None) == 0
    assert int(a["npts"].max()) > J + 2
    _compare(a, s, K, cap)
    assert s["launches"][plan] >= 2, s["launches"]
